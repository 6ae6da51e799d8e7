"""The frame's fast path with pixel-major (PX) intermediate volumes and one column per wave in the vertical passes
(stm_k_pq_hc's PX stores, stm_k_pq_v12r, stm_k_pq_hsr's PX loads, the per-column window table).

Every comparison is element for element: the default build against the CPU oracle, and against the same call under
stm_set_agg_variant(20000000), which keeps the PQ layout and the four-column kernel stm_k_pq_v12q end to end."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PQ_END_TO_END = 20000000  # the PQ layout and stm_k_pq_v12q
STANDALONE_TABLES = 1000000000  # the window tables from the stand-alone kernels instead of stm_k_cross_arms


def _run(sbs, p, stages, H, W, variant=0):
    import torch
    import stm_amd
    from stm_amd import device_api as dev
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


def _oracle(orc, sbs, p, H, W):
    return orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd,
                            p.usd, p.lsd, p.thresh_s, p.thresh_h)


def _on_px(p, H, W, stages, variant):
    """stm_agg_path: whether the dispatcher puts this call on the PX layout under `variant`"""
    import stm_amd
    from stm_amd import device_api as dev
    stm_amd.lib().stm_set_agg_variant(variant)
    try:
        return bool(dev.agg_path(p.num_disp, p.zero_disp, H, W, p.usd, stages) & dev.AGG_PX)
    finally:
        stm_amd.lib().stm_set_agg_variant(0)


def _check_frame(orc, sbs, p, H, W, variants=(0, PQ_END_TO_END), px=True):
    """stages = 1 (raw WTA maps) and stages = 3 (the finished frame) of every variant against the oracle -- and so against
    each other, bit for bit.  px: whether the case is one for the PX layout; the dispatcher is asked (stm_agg_path), so that a
    change of its conditions cannot move a case off the path it is here for without failing it."""
    want = _oracle(orc, sbs, p, H, W)
    for variant in variants:
        for stages in (1, 3):
            assert _on_px(p, H, W, stages, variant) == (px and variant != PQ_END_TO_END), "PX, variant %d" % variant
        w_l, w_r, _ = _run(sbs, p, 1, H, W, variant)
        assert np.array_equal(w_l, want["wta_l"].astype(np.float32)), "wta_l, variant %d" % variant
        assert np.array_equal(w_r, want["wta_r"].astype(np.float32)), "wta_r, variant %d" % variant
        dl, dr, out = _run(sbs, p, 3, H, W, variant)
        assert np.array_equal(dl, want["disp_l"]) and np.array_equal(dr, want["disp_r"]), "disparities, variant %d" % variant
        assert np.array_equal(out, want["interlaced"]), "interlaced, variant %d" % variant


def _params(D, usd=34, lsd=17):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=D // 2, usd=usd, lsd=lsd)


@pytest.mark.parametrize("shape", [(37, 67), (9, 13), (16, 16), (100, 193), (53, 260)])
def test_ragged_frames(gpu_ready, orc, shape):
    """D = 64, usd 34 / lsd 17.  37 x 67: H % 16 != 0, W % 4 != 0 (one padding column); 9 x 13: less than one tile each way;
    16 x 16: exactly one tile; 100 x 193: one pixel past a 192-pixel segment of stm_k_pq_hc; 53 x 260: several row parts of
    stm_k_pq_hsr."""
    from stm_amd import synth
    H, W = shape
    p = _params(64)
    sbs, _ = synth.sbs_frame(H, W, p.num_disp, p.zero_disp)
    _check_frame(orc, sbs, p, H, W)


@pytest.mark.parametrize("D", [50, 49, 48, 80])
def test_hypothesis_counts(gpu_ready, orc, D):
    """D = 50 and 49: hypotheses >= D in the last chunk of a PX pixel (zeros that must never win).  D = 48 and 80: three and five
    chunks, the PQ path as before."""
    from stm_amd import synth
    H, W = 37, 67
    p = _params(D)
    sbs, _ = synth.sbs_frame(H, W, p.num_disp, p.zero_disp)
    _check_frame(orc, sbs, p, H, W, px=D in (50, 49))


@pytest.mark.parametrize("arms", [(36, 18), (1, 1), (37, 18)])
def test_arm_limits(gpu_ready, orc, arms):
    """usd = 36: the full 88-row range of a tile's sweep; usd = 1: windows of at most two rows; usd = 37: past the register
    rings' range, stm_k_pq_v12t and the PQ layout."""
    from stm_amd import synth
    H, W = 70, 40
    p = _params(64, usd=arms[0], lsd=arms[1])
    sbs, _ = synth.sbs_frame(H, W, p.num_disp, p.zero_disp)
    _check_frame(orc, sbs, p, H, W, px=arms[0] <= 36)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_seeds(gpu_ready, orc, seed):
    from stm_amd import synth
    H, W = 64, 96
    p = _params(64)
    sbs, _ = synth.sbs_frame(H, W, p.num_disp, p.zero_disp, seed=seed)
    _check_frame(orc, sbs, p, H, W)


def test_bud_pair(gpu_ready, orc):
    """The bud_2 / bud_3 fixture pair at its own 640 x 384: real arms, long sweeps."""
    from conftest import GOLDEN
    from stm_amd import bmp_io
    L, R = bmp_io.read_bmp(os.path.join(GOLDEN, "bud_2.bmp")), bmp_io.read_bmp(os.path.join(GOLDEN, "bud_3.bmp"))
    H, W = 384, 640
    assert L.shape == (H, W, 3) and R.shape == (H, W, 3)
    sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
    _check_frame(orc, sbs, _params(64), H, W)


@pytest.mark.parametrize("shape", [(37, 67), (100, 193)])
def test_standalone_table_builders(gpu_ready, orc, shape):
    """The window tables of the stand-alone kernels (stm_k_vcol_table, stm_k_hwin_table) give the frame that the tables from
    stm_k_cross_arms give."""
    from stm_amd import synth
    H, W = shape
    p = _params(64)
    sbs, _ = synth.sbs_frame(H, W, p.num_disp, p.zero_disp)
    _check_frame(orc, sbs, p, H, W, variants=(STANDALONE_TABLES, 0))


def test_second_frame_in_the_same_workspace(gpu_ready, orc):
    """A frame of other content right after the first, same shape, same workspace: whatever the first left in the volumes'
    padding columns [W, 4G), in rows past H of a tile, or in the tables must not reach the second."""
    from stm_amd import synth
    H, W = 37, 67
    p = _params(64)
    first, _ = synth.sbs_frame(H, W, p.num_disp, p.zero_disp, seed=5)
    second, _ = synth.sbs_frame(H, W, p.num_disp, p.zero_disp, seed=6)
    assert not np.array_equal(first, second)
    want = _oracle(orc, second, p, H, W)
    for variant in (0, PQ_END_TO_END):
        _run(first, p, 3, H, W, variant)
        dl, dr, out = _run(second, p, 3, H, W, variant)
        assert np.array_equal(dl, want["disp_l"]) and np.array_equal(dr, want["disp_r"]), "disparities, variant %d" % variant
        assert np.array_equal(out, want["interlaced"]), "interlaced, variant %d" % variant
