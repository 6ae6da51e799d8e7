"""Region voting's dispatch, pinned through stm_irv_path (include/stm_hip.h): pruning, column runs, the frame's short chain, the
edge of the dirty tiles and the forced chunk of stm_set_irv_chunk.  Host arithmetic only -- nothing is launched, no GPU is needed.

The expected values are derived from irv_plan as it stands (stm_kernels_refine.hip):
  prune    no paper ratio, W <= 16000
  runs     variant digit != 3, H < 2^14, W < 2^16
  chain    a frame call, prune, runs, at least one vote, variant digit != 6, 65 + 2 usd <= 224 (usd <= 79), 14 W + 4 <= 65536 (W <= 4680)
  tile_sh  the smallest s >= 4 with 2 min(usd, 255) / 2^s + 2 <= 8, i.e. 4 up to usd 55, 5 up to 111, 6 up to 223, then 7 -- the
           frame's value, whose arms never exceed usd.  (The vote kernel's comment once said "16 x 16 for usd <= 48"; the formula
           never did: 2 * 49 / 16 + 2 = 8.)  A per-stage call votes over the caller's arm table, whose horizontal arms are bytes
           that nothing clamps, so its dirty box is the image row's part of [x - 255, x + 255] and s also satisfies
           min(510, W - 1) / 2^s + 2 <= 8: 4 up to W 112, 5 up to 224, 6 up to 448, then 7.
"""
import pytest

PRUNE, RUNS, CHAIN = 1, 2, 4
RASTER, SEPARATE = 300, 600


@pytest.fixture
def path(stm):
    from stm_amd import device_api as dev
    return dev.irv_path


def _sh(v):
    return (v >> 8) & 0xf


def _chunk(v):
    return (v >> 16) & 0x1f


def frame(path, H, W, usd, iterations=5):
    return path(H, W, usd, iterations, True, True)


def test_the_benchmark_frame(path):
    """1080 x 1920, usd 34, five iterations: pruned, column runs, the short chain, 16 x 16 tiles, no forced chunk -- the whole value"""
    assert frame(path, 1080, 1920, 34) == PRUNE | RUNS | CHAIN | (4 << 8)


@pytest.mark.parametrize("usd, sh", [(1, 4), (17, 4), (34, 4), (48, 4), (49, 4), (55, 4), (56, 5), (79, 5), (111, 5), (112, 6), (223, 6),
                                     (224, 7), (255, 7), (300, 7)])
def test_frame_tile_size_follows_usd_alone(path, usd, sh):
    """the frame's dirty tiles: as they were before the per-stage box was widened, whatever the frame's width"""
    for H, W in [(170, 70), (6, 40), (1080, 1920), (40, 4000)]:
        v = frame(path, H, W, usd)
        assert _sh(v) == sh, hex(v)
        assert bool(v & CHAIN) == (usd <= 79) and v & PRUNE and v & RUNS, hex(v)


@pytest.mark.parametrize("usd, chain", [(78, True), (79, True), (80, False), (81, False)])
def test_chain_ends_where_the_column_sums_leave_lds(path, usd, chain):
    assert frame(path, 170, 70, usd) == PRUNE | RUNS | (CHAIN if chain else 0) | (5 << 8)


@pytest.mark.parametrize("W, chain", [(4680, True), (4681, False)])
def test_chain_ends_where_the_row_kernel_leaves_lds(path, W, chain):
    assert frame(path, 6, W, 17) == PRUNE | RUNS | (CHAIN if chain else 0) | (4 << 8)


@pytest.mark.parametrize("W, prune", [(16000, True), (16001, False)])
def test_pruning_ends_at_16000_columns(path, W, prune):
    assert frame(path, 6, W, 17) == (PRUNE if prune else 0) | RUNS | (4 << 8)
    assert path(6, W, 17, 5, True, False) == (PRUNE if prune else 0) | RUNS | (7 << 8)


@pytest.mark.parametrize("H, W, runs", [(16383, 8, True), (16384, 8, False), (4, 65535, True), (4, 65536, False)])
def test_column_runs_end_where_an_entry_cannot_hold_the_pixel(path, H, W, runs):
    v = frame(path, H, W, 17)
    assert bool(v & RUNS) == runs, hex(v)
    assert bool(v & PRUNE) == (W <= 16000) and bool(v & CHAIN) == (runs and W <= 4680), hex(v)


def test_variants(stm, path):
    lib = stm.lib()
    want = {0: PRUNE | RUNS | CHAIN, RASTER: PRUNE, SEPARATE: PRUNE | RUNS}
    for variant in (RASTER, SEPARATE, 0):
        lib.stm_set_agg_variant(variant)
        try:
            got = frame(path, 80, 192, 17), path(64, 64, 17, 5, True, False)
        finally:
            lib.stm_set_agg_variant(0)
        assert got[0] == want[variant] | (4 << 8), (variant, hex(got[0]))
        assert got[1] == (want[variant] & ~CHAIN) | (4 << 8), (variant, hex(got[1]))


def test_paper_ratio_takes_pruning_and_with_it_the_chain(stm, path):
    lib = stm.lib()
    lib.stm_set_irv_paper_ratio(1)
    try:
        got = frame(path, 80, 192, 17), path(64, 64, 17, 5, True, False)
    finally:
        lib.stm_set_irv_paper_ratio(0)
    assert got == (RUNS | (4 << 8), RUNS | (4 << 8))
    assert frame(path, 80, 192, 17) == PRUNE | RUNS | CHAIN | (4 << 8)


def test_no_chain_without_the_check_or_without_a_vote(path):
    assert path(80, 192, 17, 5, True, False) == PRUNE | RUNS | (5 << 8)  # per stage: no L/R check in front
    assert path(80, 192, 17, 0, True, True) == PRUNE | RUNS | (4 << 8)   # no iteration: only the L/R check runs
    assert path(80, 192, 17, 0, False, True) == PRUNE | RUNS | (4 << 8)
    assert path(80, 192, 17, 1, True, True) == PRUNE | RUNS | CHAIN | (4 << 8)


def test_host_flavour(path):
    """dr_irv: one vote whatever `iterations` says; the same kernels, the same tiles"""
    for it in (1, 5):
        assert path(64, 64, 17, it, False, False) == path(64, 64, 17, it, True, False) == PRUNE | RUNS | (4 << 8)


@pytest.mark.parametrize("W, sh", [(48, 4), (64, 4), (112, 4), (113, 5), (200, 5), (224, 5), (225, 6), (448, 6), (449, 7), (1920, 7)])
def test_per_stage_tiles_bound_a_byte_wide_arm(path, W, sh):
    """a caller's arm table: the dirty box spans the image row's part of [x - 255, x + 255] in at most 8 tiles"""
    for usd in (4, 17, 34):
        assert _sh(path(8, W, usd, 5, True, False)) == sh
    assert _sh(path(8, W, 120, 5, True, False)) == max(sh, 6)  # never finer than the vertical box wants
    assert _sh(frame(path, 8, W, 34)) == 4


@pytest.mark.parametrize("entries", [1, 2, 3, 5, 16])
def test_forced_chunk_is_echoed(stm, path, entries):
    lib = stm.lib()
    assert lib.stm_set_irv_chunk(entries) == 0
    try:
        got = frame(path, 80, 192, 17), path(64, 64, 17, 5, True, False), path(64, 64, 17, 5, False, False)
        lib.stm_set_agg_variant(RASTER)
        try:
            raster = path(64, 64, 17, 5, True, False)
        finally:
            lib.stm_set_agg_variant(0)
    finally:
        assert lib.stm_set_irv_chunk(0) == 0
    assert got == (PRUNE | RUNS | CHAIN | (4 << 8) | (entries << 16), PRUNE | RUNS | (4 << 8) | (entries << 16),
                   PRUNE | RUNS | (4 << 8) | (entries << 16))
    assert _chunk(got[0]) == entries
    assert raster == PRUNE | (4 << 8)  # the raster vote kernel takes no chunk
    assert _chunk(frame(path, 80, 192, 17)) == 0


@pytest.mark.parametrize("entries", [17, -1, 32, 1 << 16])
def test_rejected_chunk_changes_nothing(stm, path, entries):
    lib = stm.lib()
    lib.stm_set_error_mode(1)
    try:
        assert lib.stm_set_irv_chunk(5) == 0
        assert lib.stm_set_irv_chunk(entries) == -1
        assert b"set_irv_chunk" in lib.stm_last_error()
        assert _chunk(path(64, 64, 17, 5, True, False)) == 5
        assert lib.stm_set_irv_chunk(0) == 0
        assert lib.stm_set_irv_chunk(entries) == -1
        assert _chunk(path(64, 64, 17, 5, True, False)) == 0
    finally:
        lib.stm_set_irv_chunk(0)
        lib.stm_set_error_mode(0)


def test_arguments_no_call_takes(path):
    """not screened, never a crash"""
    for H, W, usd, it in [(0, 0, 0, 0), (-3, -7, -1, -2), (1, 1, 0, 1), (1 << 20, 1 << 20, 1 << 20, 1 << 20)]:
        v = path(H, W, usd, it, True, True)
        assert 4 <= _sh(v) <= 7 and v >> 21 == 0, hex(v)
