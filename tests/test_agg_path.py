"""The frame's aggregation dispatch, pinned through stm_agg_path (include/stm_hip.h): which arguments take the pixel-major (PX) fast
path, which of stm_k_pq_hc's two instantiations its first pass runs, and from which width on a row is split over several blocks.
Host arithmetic only -- nothing is launched, no GPU is needed.

The expected values are derived from the dispatcher as it stands (stm_kernels_aggm.hip: aggm_supports, hc_waves, chain_px,
row_split).  At D = 64 hc_waves' LDS budget of 80 KB holds the 12-wave form for pad = max(zd, 63 - zd) + 15 <= 60 when the halo is
HG = 10 groups (usd 29..36) and for pad <= 188 when HG = 8 (usd 21..28), where the 16 * 12 + 2 pad <= 768 staging limit never binds
before the 8-wave form's own 128 + 2 pad <= 512 does (pad <= 192).  A retune of that budget must come here and to the cases of
tests/test_gpu_px_forms.py that name a form, instead of silently moving them onto another kernel."""
import pytest

MP, PX, VREGS, HREGS, SPLIT = 1, 2, 4, 8, 1 << 16
PQ_END_TO_END, LDS_ROW_WALK, VECTOR_ALU, SEPARATE_COST = 20000000, 100000000, 10000, 1000000


@pytest.fixture
def path(stm):
    from stm_amd import device_api as dev
    return dev.agg_path


def _waves(v):
    return (v >> 8) & 0xff


def test_the_benchmark_frame(path):
    """1080 x 1920, D 64, zd 32, usd 34, stages 3: everything on, 12 waves, one block per row -- the whole value, bit for bit"""
    assert path(64, 32, 1080, 1920, 34, 3) == MP | PX | VREGS | HREGS | (12 << 8)


@pytest.mark.parametrize("zd, usd, waves", [(17, 34, 8), (18, 34, 12), (45, 34, 12), (46, 34, 8),
                                            (17, 28, 12), (18, 28, 12), (45, 28, 12), (46, 28, 12),
                                            (0, 34, 8), (63, 34, 8), (32, 29, 12), (0, 29, 8), (0, 36, 8), (32, 36, 12)])
def test_zero_disp_selects_the_first_pass_form(path, zd, usd, waves):
    v = path(64, zd, 37, 67, usd, 3)
    assert v & PX and _waves(v) == waves, hex(v)


@pytest.mark.parametrize("zd, px", [(177, True), (178, False), (-114, True), (-115, False)])
def test_zero_disp_staging_limit(path, zd, px):
    """pad = 192 is the last that the 8-wave form's 512 threads can stage; past it the chain leaves stm_k_pq_hc and with it PX"""
    v = path(64, zd, 24, 150, 34, 1)
    assert bool(v & PX) == px and _waves(v) == (8 if px else 0), hex(v)
    assert v & MP and v & VREGS and v & HREGS, hex(v)


@pytest.mark.parametrize("D, px", [(48, False), (49, True), (64, True), (65, False)])
def test_num_disp_boundaries(path, D, px):
    v = path(D, D // 2, 37, 67, 34, 3)
    assert bool(v & PX) == px, hex(v)
    assert v & MP and v & VREGS, hex(v)
    assert bool(v & HREGS) == (D <= 64), hex(v)


@pytest.mark.parametrize("usd, px", [(1, True), (36, True), (37, False)])
def test_usd_boundaries(path, usd, px):
    v = path(64, 32, 70, 40, usd, 3)
    assert bool(v & PX) == px and bool(v & VREGS) == px and v & MP, hex(v)


@pytest.mark.parametrize("stages, px", [(1, True), (2, True), (3, True), (3 | 0x100, False), (3 | 0x200, False), (3 | 0x400, True),
                                        (3 | 0x800, True), (2 | 0x2000, True), (3 | 0x1000, True), (3 | 0x600, False)])
def test_stage_bits(path, stages, px):
    """0x100 (the scanline stage reads the aggregated volume) and 0x200 (the sub-pixel step reads the last pass's input) keep the PQ
    layout; no other bit reaches the aggregation"""
    v = path(64, 32, 40, 72, 34, stages)
    assert bool(v & PX) == px and v & MP, hex(v)
    assert bool(v & HREGS) == (not stages & 0x100), hex(v)


@pytest.mark.parametrize("variant, mp", [(PQ_END_TO_END, True), (LDS_ROW_WALK, True), (VECTOR_ALU, False), (SEPARATE_COST, True)])
def test_variants_off_px(stm, path, variant, mp):
    lib = stm.lib()
    assert path(64, 32, 40, 72, 34, 3) & PX
    lib.stm_set_agg_variant(variant)
    try:
        v = path(64, 32, 40, 72, 34, 3)
    finally:
        lib.stm_set_agg_variant(0)
    assert not v & PX and bool(v & MP) == mp, hex(v)
    if variant == PQ_END_TO_END:
        assert v == MP | VREGS | HREGS | (12 << 8)  # the same three kernels, stm_k_pq_v12q in the middle
    if variant == VECTOR_ALU:
        assert v == 0
    if variant == SEPARATE_COST:
        assert _waves(v) == 0
    assert path(64, 32, 40, 72, 34, 3) & PX


@pytest.mark.parametrize("W, zd, waves, split", [(3072, 0, 8, False), (3073, 0, 8, True), (4608, 32, 12, False), (4609, 32, 12, True),
                                                 (3100, 0, 8, True), (4700, 32, 12, True), (3840, 0, 8, True), (3840, 32, 12, False)])
def test_row_split(path, W, zd, waves, split):
    """more than 24 segments in a row: 24 * 128 columns with the 8-wave form, 24 * 192 with the 12-wave form"""
    v = path(64, zd, 3, W, 34, 3)
    assert v & PX and _waves(v) == waves and bool(v & SPLIT) == split, hex(v)


def test_arguments_no_frame_takes(path):
    """not screened, never a crash: 0 wherever the matrix-pipe chain does not run"""
    assert path(0, 0, 10, 10, 34, 3) == 0 and path(64, 32, 0, 10, 34, 3) == 0 and path(64, 32, 10, 0, 34, 3) == 0
    assert path(64, 32, 10, 10, 0, 3) == 0
