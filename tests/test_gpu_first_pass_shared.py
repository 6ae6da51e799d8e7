"""stm_k_pq_hc2: the frame's first horizontal pass with both views swept from one ring of left-referenced costs.

Every case first asserts through stm_first_pass_path that the shared kernel runs, then compares the raw WTA maps (stages = 1) element
for element with the CPU oracle and with the same call under stm_set_agg_variant(2000000), where stm_k_pq_hc evaluates each view's
costs on its own.  No tolerance anywhere.  usd 34 / lsd 17 unless a case says otherwise; an oracle frame is computed once per case."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEPARATE_VIEWS = 2000000


def _params(D, zd, usd=34, lsd=17):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd)


def _run(sbs, p, stages, variant=0):
    import torch
    import stm_amd
    from stm_amd import device_api as dev
    H, W = sbs.shape[0], sbs.shape[1] // 2
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    stm_amd.lib().stm_set_agg_variant(variant)
    try:
        dev.d_adcensus_stm(torch.from_numpy(sbs).cuda(), dl, dr, out, p, stages=stages)
        torch.cuda.synchronize()
    finally:
        stm_amd.lib().stm_set_agg_variant(0)
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _oracle(orc, sbs, p):
    H, W = sbs.shape[0], sbs.shape[1] // 2
    return orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd,
                            p.usd, p.lsd, p.thresh_s, p.thresh_h)


def _shared_runs(p, H, W, stages, parts=None):
    """stm_k_pq_hc2 runs this call (in `parts` blocks per row, if given), and stm_k_pq_hc does under SEPARATE_VIEWS"""
    import stm_amd
    from stm_amd import device_api as dev
    got = dev.first_pass_path(p.num_disp, p.zero_disp, H, W, p.usd, stages)
    assert got > 0 and (parts is None or got == parts), got
    stm_amd.lib().stm_set_agg_variant(SEPARATE_VIEWS)
    try:
        assert dev.first_pass_path(p.num_disp, p.zero_disp, H, W, p.usd, stages) == 0
    finally:
        stm_amd.lib().stm_set_agg_variant(0)


def _check(orc, sbs, p, parts=None, frame=False):
    """stages = 1 under both variants against the oracle's WTA maps; frame: also stages = 3, the interlaced frame included"""
    H, W = sbs.shape[0], sbs.shape[1] // 2
    want = _oracle(orc, sbs, p)
    _shared_runs(p, H, W, 1, parts)
    for variant in (0, SEPARATE_VIEWS):
        dl, dr, _ = _run(sbs, p, 1, variant)
        assert np.array_equal(dl, want["wta_l"].astype(np.float32)), "wta_l, variant %d" % variant
        assert np.array_equal(dr, want["wta_r"].astype(np.float32)), "wta_r, variant %d" % variant
    if frame:
        _shared_runs(p, H, W, 3, parts)
        for variant in (0, SEPARATE_VIEWS):
            dl, dr, out = _run(sbs, p, 3, variant)
            assert np.array_equal(dl, want["disp_l"]) and np.array_equal(dr, want["disp_r"]), "disparities, variant %d" % variant
            assert np.array_equal(out, want["interlaced"]), "interlaced, variant %d" % variant


def _frame(H, W, D, zd, seed_off=0):
    from stm_amd import synth
    return synth.sbs_frame(H, W, D, zd, seed=synth.SEED + seed_off)[0]


@pytest.mark.parametrize("shape", [(3, 97), (5, 100)])
@pytest.mark.parametrize("zd", [18, 45, 32])
def test_borders_dominate(gpu_ready, orc, shape, zd):
    """rows of about 100 pixels with shears of up to 45 either way: more than a sixth of the right view's costs are T at positions
    outside the row, where the left index is the clamped one"""
    H, W = shape
    _check(orc, _frame(H, W, 64, zd, 1), _params(64, zd), parts=1)


@pytest.mark.parametrize("W", [95, 96, 97, 191, 193, 260, 300, 515])
def test_segment_edges_and_ring_wrap(gpu_ready, orc, W):
    """one pixel either side of one and two 96-pixel segments; 260 and 300: the ring's 256 positions wrap and the three positions
    behind its end are read; 515: six segments in one block, the ring replaced twice over"""
    _check(orc, _frame(2, W, 64, 32, 2), _params(64, 32), parts=1, frame=(W == 300))


def test_row_parts(gpu_ready, orc):
    """700 columns are eight segments: two blocks per row, the second starting at segment 4 with a ring fill of its own"""
    _check(orc, _frame(2, 700, 64, 32, 3), _params(64, 32), parts=2)


@pytest.mark.parametrize("shape", [(64, 4), (4, 64)])
def test_fewer_hypotheses(gpu_ready, orc, shape):
    """D = 49, zd = 20: hypotheses 49..63 are zeros in the ring and the shear spans 48, not 63"""
    H, W = shape
    _check(orc, _frame(H, W, 49, 20, 4), _params(49, 20), parts=1)


@pytest.mark.parametrize("image", ["constant", "noise"])
def test_arm_extremes(gpu_ready, orc, image):
    """a constant image: every arm at usd, every window at its widest, every WTA a tie; uniform noise: arms near zero"""
    H, W = 4, 300
    if image == "constant":
        sbs = np.full((H, 2 * W, 3), 128, np.uint8)
    else:
        sbs = np.random.RandomState(5).randint(0, 256, size=(H, 2 * W, 3)).astype(np.uint8)
    _check(orc, sbs, _params(64, 32), parts=1)


@pytest.mark.parametrize("usd, lsd", [(29, 14), (36, 18)])
def test_arm_limits(gpu_ready, orc, usd, lsd):
    """usd = 29: the shortest arms with the halo of ten groups; usd = 36: the longest the kernel takes"""
    _check(orc, _frame(4, 300, 64, 32, 6), _params(64, 32, usd, lsd), parts=1)


@pytest.mark.parametrize("H", [1, 17])
def test_rows(gpu_ready, orc, H):
    _check(orc, _frame(H, 200, 64, 32, 7), _params(64, 32), parts=1)


def test_nv12_entry(gpu_ready, orc):
    """stm_d_adcensus_stm_nv12 at 6 x 200 dispatches through the same chain: equal to the BGR frame of the converted picture under
    both variants, and that frame equal to the oracle"""
    import torch
    import stm_amd
    from stm_amd import device_api as dev, synth
    from test_nv12_ref import nv12_to_bgr_ref
    H, W = 6, 200
    p = _params(64, 32)
    _shared_runs(p, H, W, 3, 1)
    y, uv = synth.bgr_to_nv12(_frame(H, W, 64, 32, 8), 0)
    bgr = nv12_to_bgr_ref(y, uv, 0)
    want = _oracle(orc, bgr, p)
    for variant in (0, SEPARATE_VIEWS):
        dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
        dr = torch.zeros_like(dl)
        out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
        il, ir = torch.zeros_like(out), torch.zeros_like(out)
        stm_amd.lib().stm_set_agg_variant(variant)
        try:
            dev.d_adcensus_stm_nv12(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), dl, dr, out, p, 3, 0, il, ir)
            torch.cuda.synchronize()
        finally:
            stm_amd.lib().stm_set_agg_variant(0)
        assert np.array_equal(dl.cpu().numpy(), want["disp_l"]) and np.array_equal(dr.cpu().numpy(), want["disp_r"]), variant
        assert np.array_equal(out.cpu().numpy(), want["interlaced"]), variant
