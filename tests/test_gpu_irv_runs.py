"""The column-run vote kernel (stm_k_irv_vote_cm) where it updates a kept histogram instead of counting a region anew.

Left to itself the kernel gives a wave max(1, min(16, n >> 14)) consecutive list entries, so below 32768 listed outliers per view
every region is counted from scratch and the signed update never runs.  stm_set_irv_chunk forces the chunk, and
tests/irv_cases.py's census says, from the inputs alone, which branch of the kernel every entry of a single-tile case takes; the
cases here are chosen so that each branch is taken often.  Every comparison is np.array_equal on the disparity and the outlier map
against the oracle (orc.dr_irv, or orc.adcensus_stm for the frame calls, whose outputs are the two disparity maps), and every test
first asks stm_irv_path whether the call is on the path the test is about.

What these tests cannot see: the kernel's `nd < nrows` (update only when fewer rows change than the region has).  Where two regions of
a column share a row and at most 64 rows change, the update gives exactly the histogram a count from scratch gives, whatever nd is; the
guard only picks the cheaper of two exact ways, so dropping it changes no output (tried on an MI355X: every test here still passes).
"""
import numpy as np
import pytest

import irv_cases
from irv_cases import census, make_case

gpu = pytest.mark.gpu
PRUNE, RUNS, CHAIN = 1, 2, 4
RASTER = 300

# single 64 x 64 tile, thresh_h = 0.0: nothing is pruned and the list's order is the census's
SINGLE = {
    "64x64": dict(H=64, W=64, D=16, zd=8, usd=17, thresh_s=12, seed=1, vmax=17, hmax=12, density=0.6, run_max=12),
    "40x33": dict(H=40, W=33, D=5, zd=2, usd=9, thresh_s=6, seed=2, vmax=9, hmax=12, density=0.6, run_max=12),
    "61x64": dict(H=61, W=64, D=16, zd=8, usd=17, thresh_s=12, seed=3, vmax=24, hmax=12, density=0.75, run_max=12),
    "7x64": dict(H=7, W=64, D=16, zd=8, usd=17, thresh_s=6, seed=4, vmax=6, hmax=5, density=0.75, run_max=4),
}
# more than one tile (the tiles append to the list through an atomic, so chunk alignment varies: no census, only the comparison)
MULTI = {
    "64x200": dict(H=64, W=200, D=16, zd=8, usd=17, thresh_s=6, thresh_h=0.0, seed=5, vmax=17, hmax=40, density=0.6, run_max=12, sh=5),
    "200x24": dict(H=200, W=24, D=16, zd=8, usd=34, thresh_s=120, thresh_h=0.0, seed=6, vmax=150, up_max=50, hmax=8, density=0.75, run_max=20,
                   sh=4),
    "130x70": dict(H=130, W=70, D=16, zd=8, usd=60, thresh_s=120, thresh_h=0.002, seed=7, vmax=60, hmax=14, density=0.75, run_max=12, sh=5),
    "75x131": dict(H=75, W=131, D=20, zd=6, usd=17, thresh_s=12, thresh_h=0.02, seed=8, vmax=17, hmax=12, density=0.6, run_max=12, sh=5),
    # arms of a table built for another usd: horizontal arms up to 31 against usd 5, in thin regions that fill up slowly, so that in
    # later iterations the only accepted pixels of a region often lie beyond [x - usd, x + usd] (the dirty box must cover them)
    "40x100_usd5": dict(H=40, W=100, D=16, zd=8, usd=5, thresh_s=35, thresh_h=0.0, seed=11, vmax=2, hmax=31, density=0.85, run_max=6, sh=4),
}
DEEP = dict(H=64, W=64, D=128, zd=64, usd=17, thresh_s=25, seed=10, vmax=17, hmax=12, density=0.75, run_max=12)
HEUR = dict(H=192, W=256, D=16, zd=8, usd=17, thresh_s=3, thresh_h=0.0, seed=11, vmax=17, hmax=12, density=0.75, run_max=24)

_GEN = ("seed", "vmax", "hmax", "density", "run_max", "up_max")
_INPUTS, _WANT = {}, {}


def inputs(c):
    key = tuple(sorted(c.items()))
    if key not in _INPUTS:
        arrs = make_case(c["H"], c["W"], c["D"], c["zd"], **{k: c[k] for k in _GEN if k in c})
        for a in arrs:
            a.setflags(write=False)
        _INPUTS[key] = arrs
    return _INPUTS[key]


def want(orc, c, iterations, device_flavour=True, paper=False):
    """the oracle's result for a case, computed once and shared read-only"""
    key = (tuple(sorted(c.items())), iterations, device_flavour, paper)
    if key not in _WANT:
        disp, outl, cross = inputs(c)
        _WANT[key] = orc.dr_irv(disp, outl, cross, c["thresh_s"], c.get("thresh_h", 0.0), c["D"], c["zd"], c["usd"], iterations,
                                device_flavour=device_flavour)
        for a in _WANT[key]:
            a.setflags(write=False)
    return _WANT[key]


def accepted_per_iteration(orc, c, iterations=5):
    left = [int((inputs(c)[1] != 0).sum())] + [int((want(orc, c, it)[1] != 0).sum()) for it in range(1, iterations + 1)]
    return [a - b for a, b in zip(left, left[1:])]


def d_dr_irv(stm, c, iterations, arrs=None):
    """stm_d_dr_irv on device copies of the case's inputs -> (disp, outliers) as numpy"""
    import torch
    from stm_amd import device_api as dev
    disp, outl, cross = arrs if arrs is not None else inputs(c)
    d, o, x = torch.from_numpy(disp.copy()).cuda(), torch.from_numpy(outl.copy()).cuda(), torch.from_numpy(cross.copy()).cuda()
    tab = dev.plane_table(x)
    dev._use_current_stream()
    lib = stm.lib()
    lib.stm_d_dr_irv(d.data_ptr(), o.data_ptr(), tab.data_ptr(), c["thresh_s"], c.get("thresh_h", 0.0), c["H"], c["W"], c["D"], c["zd"],
                     c["usd"], iterations)
    torch.cuda.synchronize()
    assert b"outlier list" not in (lib.stm_last_error() or b"")
    assert torch.equal(x.cpu(), torch.from_numpy(cross.copy()))
    return d.cpu().numpy(), o.cpu().numpy()


def same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


class forced:
    """stm_set_irv_chunk(entries) for a block, the kernel's own rule afterwards"""

    def __init__(self, stm, entries):
        self.lib, self.entries = stm.lib(), entries

    def __enter__(self):
        assert self.lib.stm_set_irv_chunk(self.entries) == 0

    def __exit__(self, *exc):
        self.lib.stm_set_irv_chunk(0)


def per_stage_path(H, W, usd, iterations, device_flavour=True):
    from stm_amd import device_api as dev
    return dev.irv_path(H, W, usd, iterations, device_flavour, False)


# ---------------------------------------------------------------- conditions on the inputs (no GPU)
def test_census_single_tile_cases_reach_every_branch():
    """chunk 16: every class of the kernel's `if` at least 10 times on at least one case (more than 64 changed rows cannot
    happen inside 64 rows: the 200 x 24 case is for that); chunks 3, 5 and 16 each leave a tail chunk on some case"""
    cen = {n: census(inputs(c)[1], inputs(c)[2], c["usd"], 16, c["thresh_s"]) for n, c in SINGLE.items()}
    for k in irv_cases.CLASSES:
        if k != "nd_gt_64":
            assert max(cn[k] for cn in cen.values()) >= 10, (k, cen)
    big = cen["64x64"]
    assert all(big[k] >= 10 for k in irv_cases.CLASSES if k != "nd_gt_64"), big  # one case alone reaches them all
    assert max(cn["later"] for cn in cen.values()) >= 10, cen  # entries that are skipped inside a chunk, the histogram kept
    for chl in (3, 5, 16):
        assert any(cn["entries"] % chl for cn in cen.values()), (chl, cen)
    one = census(inputs(SINGLE["64x64"])[1], inputs(SINGLE["64x64"])[2], 17, 1, SINGLE["64x64"]["thresh_s"])
    assert one["first"] + one["later"] == one["entries"]  # chunk 1, the control: nothing but counts from scratch


def test_census_updates_survive_in_small_chunks():
    for chl, least in ((2, 100), (3, 150), (5, 200)):
        c = SINGLE["64x64"]
        cn = census(inputs(c)[1], inputs(c)[2], c["usd"], chl, c["thresh_s"])
        assert cn["remove_only"] + cn["add_only"] + cn["both"] >= least, (chl, cn)


@pytest.mark.parametrize("name", list(SINGLE) + list(MULTI))
def test_oracle_accepts_in_at_least_three_iterations(orc, name):
    """so iterations 2 and later (the dirty-tile skip, IV_ACCEPTED entries inside chunks, both code planes) decide results"""
    c = SINGLE.get(name) or MULTI[name]
    acc = accepted_per_iteration(orc, c)
    assert sum(1 for a in acc if a > 0) >= 3 and acc[0] >= 10, acc


def test_multi_tile_inputs_hold_what_they_are_for():
    c = MULTI["64x200"]
    _, outl, cross = inputs(c)
    for lo in (32, 64):  # rows wider than half a wave / a whole wave, entering and leaving a region along a vertical outlier run
        enter, leave = irv_cases.wide_rows_in_runs(outl, cross, c["usd"], lo)
        assert enter >= 50 and leave >= 50, (lo, enter, leave)
    c = MULTI["200x24"]
    _, outl, cross = inputs(c)
    H = c["H"]
    big = runs_over_edge = 0
    for x in range(c["W"]):
        for y in range(H - 1):
            if outl[y, x] and outl[y + 1, x]:
                a0, a1 = irv_cases.region_rows(cross, y, x, H, c["usd"])
                b0, b1 = irv_cases.region_rows(cross, y + 1, x, H, c["usd"])
                nd = abs(a0 - b0) + abs(a1 - b1)
                big += max(a0, b0) <= min(a1, b1) and 64 < nd < b1 - b0 + 1
                runs_over_edge += y % 64 == 63
    assert big >= 10 and runs_over_edge >= 10, (big, runs_over_edge)  # nd > 64 with nd < nrows; runs that cross a tile's lower edge
    assert int(cross[0].max()) > c["usd"]  # the up arm's clamp to usd decides rows


def test_heuristic_case_lists_enough_for_two_entries_per_wave():
    """thresh_h = 0.0 prunes nothing, so every outlier is listed: 32768 <= n < 49152 gives chl = n >> 14 = 2 without the seam"""
    n = int((inputs(HEUR)[1] != 0).sum())
    assert 32768 <= n <= 49151 and n >> 14 == 2, n


# ---------------------------------------------------------------- per-stage calls, one view
@gpu
@pytest.mark.parametrize("chunk", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("name", list(SINGLE))
def test_single_tile_forced_chunk(gpu_ready, stm, orc, name, chunk):
    """d_dr_irv with 1 and 5 iterations and dr_irv (host flavour: one vote) under every chunk; chunk 1 is the control"""
    from stm_amd import host_api
    c = SINGLE[name]
    disp, outl, cross = inputs(c)
    with forced(stm, chunk):
        for it in (1, 5):
            assert per_stage_path(c["H"], c["W"], c["usd"], it) == PRUNE | RUNS | (4 << 8) | (chunk << 16)
            assert same(d_dr_irv(stm, c, it), want(orc, c, it)), "d_dr_irv, %d iterations" % it
        assert per_stage_path(c["H"], c["W"], c["usd"], 5, False) == PRUNE | RUNS | (4 << 8) | (chunk << 16)
        got = host_api.dr_irv(disp, outl, cross, c["thresh_s"], 0.0, c["D"], c["zd"], c["usd"], 5)
        assert same(got, want(orc, c, 5, device_flavour=False)), "dr_irv"


@gpu
@pytest.mark.parametrize("name", list(MULTI))
def test_multi_tile_forced_chunk_16(gpu_ready, stm, orc, name):
    c = MULTI[name]
    with forced(stm, 16):
        for it in (1, 5):
            assert per_stage_path(c["H"], c["W"], c["usd"], it) == PRUNE | RUNS | (c["sh"] << 8) | (16 << 16)
            assert same(d_dr_irv(stm, c, it), want(orc, c, it)), "%d iterations" % it


@gpu
@pytest.mark.parametrize("chunk", [1, 16])
def test_more_than_65_bins(gpu_ready, stm, orc, chunk):
    """D 128: the histogram's clear, its update and its final walk take several trips per lane"""
    assert sum(1 for a in accepted_per_iteration(orc, DEEP) if a > 0) >= 3
    assert len(np.unique(want(orc, DEEP, 5)[0])) > 65
    with forced(stm, chunk):
        assert per_stage_path(64, 64, 17, 5) == PRUNE | RUNS | (4 << 8) | (chunk << 16)
        assert same(d_dr_irv(stm, DEEP, 5), want(orc, DEEP, 5))


@gpu
def test_paper_ratio_with_forced_chunk(gpu_ready, stm, orc):
    """the paper's accept rule: no pruning, no early retirement of entries, so every outlier stays in the chunks for 5 iterations"""
    c = dict(SINGLE["64x64"], thresh_h=0.3)
    lib = stm.lib()
    lib.stm_set_irv_paper_ratio(1)
    orc.set_irv_paper_ratio(1)
    try:
        exp = want(orc, c, 5, paper=True)
        with forced(stm, 16):
            assert per_stage_path(64, 64, 17, 5) == RUNS | (4 << 8) | (16 << 16)
            got = d_dr_irv(stm, c, 5)
    finally:
        lib.stm_set_irv_paper_ratio(0)
        orc.set_irv_paper_ratio(0)
    assert same(got, exp)
    plain = want(orc, c, 5)
    assert (exp[1] != 0).sum() not in (0, (inputs(c)[1] != 0).sum()) and not np.array_equal(exp[1], plain[1])  # the rule decides here


@gpu
def test_raster_list_ignores_the_chunk(gpu_ready, stm, orc):
    """stm_set_agg_variant(300): the raster list and stm_k_irv_vote, on which a forced chunk is inert"""
    c = SINGLE["64x64"]
    lib = stm.lib()
    lib.stm_set_agg_variant(RASTER)
    try:
        with forced(stm, 16):
            assert per_stage_path(64, 64, 17, 5) == PRUNE | (4 << 8)
            got = d_dr_irv(stm, c, 5)
    finally:
        lib.stm_set_agg_variant(0)
    assert same(got, want(orc, c, 5))


@gpu
def test_kernels_own_chunk_of_two(gpu_ready, stm, orc):
    """no seam: 192 x 256 with three outliers in four pixels lists more than 32768 of them, the smallest shape at which the
    shipped rule leaves one entry per wave"""
    c = HEUR
    assert 32768 <= int((inputs(c)[1] != 0).sum()) <= 49151
    assert per_stage_path(c["H"], c["W"], c["usd"], 5) == PRUNE | RUNS | (6 << 8)
    assert sum(1 for a in accepted_per_iteration(orc, c) if a > 0) >= 3
    assert same(d_dr_irv(stm, c, 5), want(orc, c, 5))


# ---------------------------------------------------------------- arms longer than usd: the dirty box
def directed_case():
    """One long right arm against usd 4.  (2, 4)'s region is row 2, columns 4 .. 34, all outliers: nothing to vote with in the
    first iteration.  (2, 29) is accepted in it (one reliable pixel below), 25 columns to the right of (2, 4) -- beyond
    [x - usd, x + usd], in the next 16-pixel tile -- and gives (2, 4) its vote in the second."""
    H, W = 8, 48
    c = dict(H=H, W=W, D=16, zd=8, usd=4, thresh_s=0, thresh_h=0.0)
    disp = np.full((H, W), 3, np.float32)
    outl = np.zeros((H, W), np.uint8)
    outl[2, 4:35] = 1
    cross = np.zeros((4, H, W), np.uint8)
    cross[3, 2, 4] = 30
    cross[1, 2, 29] = 1
    return c, (disp, outl, cross)


@gpu
@pytest.mark.parametrize("variant", [0, RASTER])
def test_accepted_pixel_beyond_usd_columns_wakes_the_outlier(gpu_ready, stm, orc, variant):
    c, arrs = directed_case()
    one = orc.dr_irv(*arrs, 0, 0.0, c["D"], c["zd"], c["usd"], 1)
    two = orc.dr_irv(*arrs, 0, 0.0, c["D"], c["zd"], c["usd"], 2)
    assert one[1][2, 29] == 0 and one[1][2, 4] == 1 and two[1][2, 4] == 0 and int((two[1] != 0).sum()) == 29
    lib = stm.lib()
    lib.stm_set_agg_variant(variant)
    try:
        assert per_stage_path(8, 48, 4, 2) == PRUNE | (0 if variant else RUNS) | (4 << 8)
        got1, got2 = d_dr_irv(stm, c, 1, arrs), d_dr_irv(stm, c, 2, arrs)
    finally:
        lib.stm_set_agg_variant(0)
    assert same(got1, one)
    assert same(got2, two)


def directed_tall_case():
    """One long down arm against usd 4, 100 columns wide (7 tile columns of 16 pixels, all inside a caller's box).  (2, 4)'s region
    is column 4, rows 2 .. 152, plus row 150's columns 4 .. 34 -- all outliers, so nothing to vote with in the first iteration.  Its
    box is 7 x 10 = 70 tiles, more than a wave has lanes.  (150, 29) is accepted in the first iteration, in the box's bottom tile row,
    tile 64 of the 70: a skip decided on the first 64 tiles alone misses it and leaves (2, 4) an outlier in the second."""
    H, W = 160, 100
    c = dict(H=H, W=W, D=16, zd=8, usd=4, thresh_s=0, thresh_h=0.0)
    disp = np.full((H, W), 3, np.float32)
    outl = np.zeros((H, W), np.uint8)
    outl[2:153, 4] = 1
    outl[150, 4:35] = 1
    cross = np.zeros((4, H, W), np.uint8)
    cross[1, 2, 4] = 150
    cross[3, 150, 4] = 30
    cross[1, 150, 29] = 1
    return c, (disp, outl, cross)


@gpu
@pytest.mark.parametrize("variant", [0, RASTER])
def test_accepted_pixel_in_a_box_of_more_than_64_tiles_wakes_the_outlier(gpu_ready, stm, orc, variant):
    c, arrs = directed_tall_case()
    one = orc.dr_irv(*arrs, 0, 0.0, c["D"], c["zd"], c["usd"], 1)
    two = orc.dr_irv(*arrs, 0, 0.0, c["D"], c["zd"], c["usd"], 2)
    assert int((arrs[1] != 0).sum()) - int((one[1] != 0).sum()) == 1 and one[1][150, 29] == 0 and one[1][2, 4] == 1
    assert two[1][2, 4] == 0 and two[1][150, 4] == 0 and int((one[1] != 0).sum()) - int((two[1] != 0).sum()) == 2
    sh, tiles_x = 4, (c["W"] + 15) // 16
    assert tiles_x * ((152 >> sh) - (2 >> sh) + 1) > 64 and (150 >> sh) * tiles_x + (29 >> sh) >= 64  # the box, the dirty tile's place in it
    lib = stm.lib()
    lib.stm_set_agg_variant(variant)
    try:
        assert per_stage_path(c["H"], c["W"], c["usd"], 2) == PRUNE | (0 if variant else RUNS) | (sh << 8)
        got1, got2 = d_dr_irv(stm, c, 1, arrs), d_dr_irv(stm, c, 2, arrs)
    finally:
        lib.stm_set_agg_variant(0)
    assert same(got1, one)
    assert same(got2, two)


@gpu
@pytest.mark.parametrize("variant", [0, RASTER])
def test_arm_table_of_another_usd(gpu_ready, stm, orc, variant):
    """horizontal arms up to 31 against usd 5, five iterations, both vote kernels"""
    c = MULTI["40x100_usd5"]
    lib = stm.lib()
    lib.stm_set_agg_variant(variant)
    try:
        with forced(stm, 16):
            assert per_stage_path(c["H"], c["W"], c["usd"], 5) == (PRUNE | (4 << 8) if variant else PRUNE | RUNS | (4 << 8) | (16 << 16))
            got = d_dr_irv(stm, c, 5)
    finally:
        lib.stm_set_agg_variant(0)
    assert same(got, want(orc, c, 5))


# ---------------------------------------------------------------- the frame's chain, two views
def heavy_frame():
    """the frame of test_gpu_parity.py::test_real_image_statistics_irv_heavy"""
    rng = np.random.RandomState(12)
    H, W = 80, 192
    L = np.kron(rng.randint(0, 256, size=(H // 4, W // 4, 3)), np.ones((4, 4, 1))).astype(np.uint8)
    R = np.roll(L, -2, axis=1).copy()
    R[:, 40:90] = rng.randint(0, 256, size=(H, 50, 3))
    return np.ascontiguousarray(np.concatenate([L, R], axis=1)), dict(num_disp=16, zero_disp=8, usd=17, lsd=8, thresh_s=5, thresh_h=0.1)


def ragged_frame(H, W, D, zd, usd, lsd, seed, thresh_s=5, thresh_h=0.1):
    rng = np.random.RandomState(seed)
    L = np.kron(rng.randint(0, 256, size=(H // 4 + 1, W // 4 + 1, 3)), np.ones((4, 4, 1)))[:H, :W].astype(np.uint8)
    R = np.roll(L, -2, axis=1).copy()
    a, b = W // 4, W // 4 + max(W // 4, 2)
    R[:, a:b] = rng.randint(0, 256, size=(H, b - a, 3))  # an unmatched band: many L/R outliers
    return (np.ascontiguousarray(np.concatenate([L, R], axis=1)),
            dict(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd, thresh_s=thresh_s, thresh_h=thresh_h))


FRAMES = {
    "heavy_80x192": (heavy_frame, ()),
    "ragged_75x131": (ragged_frame, (75, 131, 20, 6, 17, 8, 21)),
    "chain_usd79_170x70": (ragged_frame, (170, 70, 16, 8, 79, 20, 22)),
    "no_chain_usd80_170x70": (ragged_frame, (170, 70, 16, 8, 80, 20, 22)),
    "chain_w4680": (ragged_frame, (6, 4680, 4, 1, 17, 8, 23, 2, 0.01)),
    "no_chain_w4681": (ragged_frame, (6, 4681, 4, 1, 17, 8, 23, 2, 0.01)),
}
_FRAME = {}


def frame_ref(orc, name):
    if name not in _FRAME:
        from stm_amd import device_api as dev
        fn, args = FRAMES[name]
        sbs, kw = fn(*args)
        p = dev.FrameParams(**kw)
        H, W = sbs.shape[0], sbs.shape[1] // 2
        w = orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd,
                             p.lsd, p.thresh_s, p.thresh_h)
        _FRAME[name] = (sbs, p, w)
    return _FRAME[name]


@gpu
@pytest.mark.parametrize("chunk", [1, 16])
@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_chain_forced_chunk(gpu_ready, stm, orc, name, chunk):
    """d_adcensus_stm, stages 2: both views through every region-voting launch, on the short chain (stm_k_dcc_irv_rows +
    stm_k_irv_compact_cm<true>) and on either side of its two limits (usd 79 / 80, W 4680 / 4681)"""
    import torch
    from stm_amd import device_api as dev
    sbs, p, w = frame_ref(orc, name)
    H, W = sbs.shape[0], sbs.shape[1] // 2
    assert (w["wta_l"] != w["disp_l"]).any() and (w["wta_r"] != w["disp_r"]).any()  # refinement decides values in both views
    chain = not name.startswith("no_chain")
    sh = 5 if p.usd >= 56 else 4
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    with forced(stm, chunk):
        assert dev.irv_path(H, W, p.usd, 5, True, True) == PRUNE | RUNS | (CHAIN if chain else 0) | (sh << 8) | (chunk << 16)
        dev.d_adcensus_stm(torch.from_numpy(sbs).cuda(), dl, dr, out, p, stages=2)
        torch.cuda.synchronize()
    assert b"outlier list" not in (stm.lib().stm_last_error() or b"")
    assert np.array_equal(dl.cpu().numpy(), w["disp_l"]) and np.array_equal(dr.cpu().numpy(), w["disp_r"])
