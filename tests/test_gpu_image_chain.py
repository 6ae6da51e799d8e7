"""The image-sized chain of the frame pipeline: the fused front kernel (split + pixel formats + census), the fused row kernel
(L/R check + reliable-pixel row counts + vote codes) and the compaction kernel that forms its column sums in LDS, against the CPU
oracle -- with the default selection (variant 0) and with the separate kernels they replace (stm_set_agg_variant(600)) -- on
shapes that hit their edges: W not a multiple of 4 or of 64, H not a multiple of 64 and smaller than usd, usd = 36, the largest
usd whose column-sum tile fits LDS (79) and one beyond it (90: the separate kernels must run and still agree), D = 20 and 130,
and frames whose left half ends and right half begins with strongly different columns (the census clamps to the edge of its
own half, never into the other half of the side-by-side row).

At stages = 2 the pipeline stops after the refined disparity maps: they are compared, and the interlaced buffer must be left
untouched; at stages = 3 all three outputs are compared."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (H, W, D, zd, usd, lsd, seam)
CASES = {
    "w203_h70_usd36_d20": (70, 203, 20, 8, 36, 18, False),
    "h30_below_usd36_d130": (30, 150, 130, 64, 36, 17, False),
    "three_tile_rows_w333": (130, 333, 64, 32, 17, 8, False),
    "usd90_beyond_lds_tile": (100, 262, 20, 8, 90, 20, False),
    "usd79_largest_lds_tile": (150, 131, 20, 10, 79, 30, False),
    "seam_w128": (72, 128, 20, 8, 17, 8, True),
    "seam_w90": (40, 90, 20, 8, 36, 12, True),
}


@functools.lru_cache(maxsize=None)
def _frame(name):
    from stm_amd import synth
    H, W, D, zd, usd, lsd, seam = CASES[name]
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=len(name) + H)
    if seam:  # the left half ends bright and noisy, the right half begins dark: a census that looked across the seam would differ
        sbs = sbs.copy()
        rng = np.random.RandomState(H * W)
        sbs[:, W - 6:W] = rng.randint(200, 256, size=(H, 6, 3)).astype(np.uint8)
        sbs[:, W:W + 6] = rng.randint(0, 40, size=(H, 6, 3)).astype(np.uint8)
    return sbs


@functools.lru_cache(maxsize=None)
def _want(name):
    from oracle import pyoracle as orc
    from stm_amd import device_api as dev
    H, W, D, zd, usd, lsd, _ = CASES[name]
    p = dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd)
    return orc.adcensus_stm(_frame(name), H, W, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, usd, lsd,
                            p.thresh_s, p.thresh_h)


@pytest.mark.parametrize("variant", [0, 600])
@pytest.mark.parametrize("stages", [2, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_image_chain_vs_oracle(gpu_ready, orc, name, stages, variant):
    import torch
    import stm_amd
    from stm_amd import device_api as dev
    H, W, D, zd, usd, lsd, _ = CASES[name]
    sbs = _frame(name)
    p = dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd)
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    stm_amd.lib().stm_set_agg_variant(variant)
    try:
        dev.d_adcensus_stm(torch.from_numpy(sbs).cuda(), dl, dr, out, p, stages=stages)
        torch.cuda.synchronize()
    finally:
        stm_amd.lib().stm_set_agg_variant(0)
    want = _want(name)
    where = (name, stages, variant)
    assert np.array_equal(dl.cpu().numpy(), want["disp_l"]), where
    assert np.array_equal(dr.cpu().numpy(), want["disp_r"]), where
    if stages >= 3:
        assert np.array_equal(out.cpu().numpy(), want["interlaced"]), where
    else:
        assert not out.cpu().numpy().any(), where

