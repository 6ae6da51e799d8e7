"""The cross-arm walk (stm_k_cross_arms, stm_kernels_agg.hip) against the CPU oracle, on shapes and parameters that hit the
edges of its addressing and bookkeeping: the walk reads up / down rows through a scalar row offset that stops at the arm's last
row, left / right pixels through a row descriptor whose range check answers for what falls off either end of the row, keeps
"arm still open" as one lane mask per direction, counts the arm up while it is open, and runs its steps in pairs with one odd
step after each tier.

Part one: the four arm planes of the per-stage call (host_api.ca_cross: the kernel without the window tables) against the
oracle's cross_arms.  Part two: the frame (the kernel with both window tables for usd <= 36 and D <= 64, with the horizontal one
alone when the vertical passes run on the LDS ring, without tables beyond that) against the oracle's adcensus_stm.  Both under
the default selection and with the previous walk, stm_set_agg_variant(700), which must give the same planes.

Shapes: W not a multiple of 4 or of 64 and beyond one 256-lane block, H not a multiple of 16, images narrower and lower than usd,
usd < lsd, usd = lsd, usd = 1 and 2, lsd = 0 and below (no near tier; odd and even), even and odd step counts in either tier, usd = 36 (the tables' range), 37, 90 and 140 (beyond
it; the per-stage call's own aggregation pass has no room in LDS for arms much longer than that), 255 (the u8 limit; part two
only, for that reason: frames of lines along which the arms take every length up to 255), thresholds -1, 0, 254.5, 255 and NaN, and frames whose border rows and columns carry strong edges."""
import functools

import numpy as np
import pytest

from conftest import rand_pair

pytestmark = pytest.mark.gpu

NAN = float("nan")

# (H, W, usd, lsd, ucd, lcd, image)   image: "rand" = conftest.rand_pair, "flat" = smooth (long arms), "edges" = rand + striped borders
ARM_CASES = {
    "defaults_w203_h70": (70, 203, 34, 17, 6.0, 20.0, "rand"),
    "two_blocks_w300_h19": (19, 300, 34, 17, 6.0, 20.0, "flat"),
    "w128_h32_multiple_of_64": (32, 128, 34, 17, 6.0, 20.0, "flat"),
    "narrower_and_lower_than_usd": (20, 25, 34, 17, 6.0, 20.0, "flat"),
    "one_pixel": (1, 1, 34, 17, 6.0, 20.0, "flat"),
    "one_row": (1, 77, 34, 17, 6.0, 20.0, "flat"),
    "one_column": (45, 1, 34, 17, 6.0, 20.0, "flat"),
    "usd_below_lsd": (37, 90, 5, 9, 6.0, 20.0, "flat"),
    "usd_equals_lsd": (37, 90, 12, 12, 6.0, 20.0, "flat"),
    "usd_1": (18, 66, 1, 1, 6.0, 20.0, "flat"),
    "usd_2_lsd_1": (18, 66, 2, 1, 6.0, 20.0, "flat"),
    "even_near_even_far": (50, 131, 34, 16, 6.0, 20.0, "flat"),
    "odd_near_even_far": (50, 131, 35, 17, 6.0, 20.0, "flat"),
    "lsd_0": (30, 70, 9, 0, 6.0, 20.0, "flat"),
    "lsd_minus_1": (30, 70, 9, -1, 6.0, 20.0, "flat"),
    "lsd_minus_2": (30, 70, 9, -2, 6.0, 20.0, "flat"),
    "lsd_minus_1_even_usd": (30, 70, 10, -1, 40.0, 20.0, "flat"),
    "lsd_minus_7_edges": (41, 67, 34, -7, 60.0, 0.0, "edges"),
    "usd_36": (75, 130, 36, 17, 6.0, 20.0, "flat"),
    "usd_37": (75, 130, 37, 18, 6.0, 20.0, "flat"),
    "usd_90": (100, 262, 90, 20, 6.0, 20.0, "flat"),
    "usd_140_arms_to_the_border": (70, 300, 140, 140, 255.0, 255.0, "rand"),
    "usd_140_far_tier": (40, 330, 140, 17, 40.0, 60.0, "flat"),
    "ucd_minus_1": (40, 99, 34, 17, -1.0, 20.0, "flat"),
    "lcd_minus_1": (40, 99, 34, 17, 6.0, -1.0, "flat"),
    "both_0": (40, 99, 34, 17, 0.0, 0.0, "flat"),
    "both_254_5": (40, 99, 34, 17, 254.5, 254.5, "edges"),
    "both_255": (40, 99, 34, 17, 255.0, 255.0, "edges"),
    "both_nan": (40, 99, 34, 17, NAN, NAN, "edges"),
    "ucd_nan": (40, 99, 34, 17, NAN, 20.0, "rand"),
    "lcd_nan_ucd_0": (40, 99, 34, 17, 0.0, NAN, "rand"),
    "border_edges_w203_h70": (70, 203, 34, 17, 6.0, 20.0, "edges"),
    "border_edges_loose": (53, 67, 36, 17, 60.0, 120.0, "edges"),
}


def _striped_borders(img):
    """Rows 0, 1, H-2, H-1 and columns 0, 1, W-2, W-1 alternate black and white: every walk that reaches a border crosses an edge
    there, and one pixel further (outside) there is nothing that may be taken for a pixel."""
    img = img.copy()
    H, W, _ = img.shape
    stripes_w = ((np.arange(W) % 2) * 255).astype(np.uint8)[:, None]
    stripes_h = ((np.arange(H) % 2) * 255).astype(np.uint8)[:, None]
    for r in (0, 1, H - 2, H - 1):
        if 0 <= r < H:
            img[r] = stripes_w if r % 2 == 0 else 255 - stripes_w
    for c in (0, 1, W - 2, W - 1):
        if 0 <= c < W:
            img[:, c] = stripes_h if c % 2 == 0 else 255 - stripes_h
    return img


def _image(H, W, kind, seed):
    if kind == "flat":  # a smooth ramp + weak noise: arms reach usd and the borders
        rng = np.random.RandomState(seed)
        y, x = np.mgrid[0:H, 0:W]
        base = np.stack([40 + x // 3 + y // 5, 90 + y // 2, 200 - x // 4], axis=-1) + rng.randint(0, 4, size=(H, W, 3))
        return np.clip(base, 0, 255).astype(np.uint8)
    L, _ = rand_pair(max(H, 8), max(W, 8), seed)
    L = np.ascontiguousarray(L[:H, :W])
    return _striped_borders(L) if kind == "edges" else L


@functools.lru_cache(maxsize=None)
def _arm_case(name):
    from oracle import pyoracle as orc
    H, W, usd, lsd, ucd, lcd, kind = ARM_CASES[name]
    img = _image(H, W, kind, 100 + H + W)
    want = orc.cross_arms(img, ucd, lcd, usd, lsd)
    want.setflags(write=False)
    return img, want


@pytest.mark.parametrize("variant", [0, 700])
@pytest.mark.parametrize("name", sorted(ARM_CASES))
def test_arm_planes_vs_oracle(gpu_ready, orc, stm, name, variant):
    from stm_amd import host_api
    H, W, usd, lsd, ucd, lcd, _ = ARM_CASES[name]
    img, want = _arm_case(name)
    cost = np.zeros((1, H, W), np.float32)
    stm.lib().stm_set_agg_variant(variant)
    try:
        got, _ = host_api.ca_cross(img, cost, ucd, lcd, usd, lsd)
    finally:
        stm.lib().stm_set_agg_variant(0)
    for d, plane in enumerate(("up", "down", "left", "right")):
        bad = np.argwhere(got[d] != want[d])
        assert bad.size == 0, (name, variant, plane, len(bad), bad[:4].tolist(), got[d][tuple(bad[0])], want[d][tuple(bad[0])])


# (H, W, D, zd, usd, lsd, ucd, lcd, frame)   frame: False = synth.sbs_frame, True = the same with striped borders, "rows" / "columns" = _line_frame
FRAME_CASES = {
    "both_tables_w203_h70_usd36": (70, 203, 20, 8, 36, 18, 6.0, 20.0, False),
    "both_tables_defaults_w131_h50": (50, 131, 20, 8, 34, 17, 6.0, 20.0, False),
    "narrower_and_lower_than_usd": (20, 30, 12, 4, 34, 17, 6.0, 20.0, False),
    "usd_below_lsd": (40, 90, 20, 8, 9, 12, 6.0, 20.0, False),
    "usd_equals_lsd": (40, 90, 20, 8, 12, 12, 6.0, 20.0, False),
    "no_tables_usd90": (100, 262, 20, 8, 90, 20, 6.0, 20.0, False),
    "no_tables_d130": (30, 150, 130, 64, 36, 17, 6.0, 20.0, False),
    "usd255": (40, 70, 12, 4, 255, 17, 6.0, 20.0, False),
    "usd255_long_left_right_arms": (48, 300, 8, 4, 255, 17, 6.0, 20.0, "rows"),
    "usd255_long_up_down_arms": (300, 48, 8, 4, 255, 17, 6.0, 20.0, "columns"),
    "lsd_minus_1": (40, 90, 20, 8, 9, -1, 6.0, 20.0, False),
    "lsd_minus_2_both_tables": (50, 131, 20, 8, 34, -2, 6.0, 20.0, False),
    "ucd_nan_lcd_255": (36, 75, 12, 4, 34, 17, NAN, 255.0, False),
    "ucd_minus_1_lcd_0": (36, 75, 12, 4, 34, 17, -1.0, 0.0, False),
    "both_254_5": (36, 75, 12, 4, 34, 17, 254.5, 254.5, False),
    "border_edges": (53, 67, 20, 8, 36, 17, 6.0, 20.0, True),
    "border_edges_loose": (53, 67, 20, 8, 36, 17, 60.0, 120.0, True),
}
# 700: the previous walk.  10000000: the vertical passes on the LDS ring, so the walk builds the horizontal table alone.
FRAME_VARIANTS = [0, 700, 10000000, 10000700]


def _line_frame(H, W, seed, columns):
    """A side-by-side frame of lines (image rows, or columns) of one colour each with weak noise, every line changing to another
    colour at a place of its own, the right view two pixels along: arms along the lines take every length up to usd = 255
    (thousands between 140 and 255 at the sizes used here), arms across them end after a pixel or two.  For the rows form the
    oracle's frame changes in 285 disparities when usd goes from 255 to 254, so the long counts do reach the
    outputs that are compared; for the columns form it does not change (the vertical window enters the result less directly),
    and that case only shows that such a walk runs and agrees."""
    rng = np.random.RandomState(seed)
    n, length = (W, H) if columns else (H, W)
    colour = rng.randint(20, 236, size=(n + 8, 3))
    other = rng.randint(20, 236, size=(n + 8, 3))
    change = rng.randint(0, length, size=n + 8)
    along = np.arange(length)[:, None]
    base = np.where((along >= change[None, :])[:, :, None], other[None, :, :], colour[None, :, :]).astype(np.int32)  # [length][n + 8][3]
    views = []
    for first in (3, 5):
        v = np.clip(base[:, first:first + n] + rng.randint(-2, 3, size=(length, n, 3)), 0, 255).astype(np.uint8)
        views.append(v if columns else v.transpose(1, 0, 2))
    return np.ascontiguousarray(np.concatenate(views, axis=1))


@functools.lru_cache(maxsize=None)
def _frame(name):
    from stm_amd import synth
    H, W, D, zd, usd, lsd, ucd, lcd, edges = FRAME_CASES[name]
    if edges in ("rows", "columns"):
        sbs = _line_frame(H, W, 3, edges == "columns")
        sbs.setflags(write=False)
        return sbs
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=len(name) + W)
    if edges:
        sbs = np.ascontiguousarray(np.concatenate([_striped_borders(sbs[:, :W]), _striped_borders(sbs[:, W:])], axis=1))
    sbs.setflags(write=False)
    return sbs


def _params(name):
    from stm_amd import device_api as dev
    H, W, D, zd, usd, lsd, ucd, lcd, _ = FRAME_CASES[name]
    return dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd, ucd=ucd, lcd=lcd)


@functools.lru_cache(maxsize=None)
def _frame_want(name):
    from oracle import pyoracle as orc
    H, W, D, zd, usd, lsd, ucd, lcd, _ = FRAME_CASES[name]
    p = _params(name)
    return orc.adcensus_stm(_frame(name), H, W, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, ucd, lcd, usd, lsd,
                            p.thresh_s, p.thresh_h)


@pytest.mark.parametrize("variant", FRAME_VARIANTS)
@pytest.mark.parametrize("name", sorted(FRAME_CASES))
def test_frame_vs_oracle(gpu_ready, orc, name, variant):
    import torch
    import stm_amd
    from stm_amd import device_api as dev
    H, W = FRAME_CASES[name][:2]
    p = _params(name)
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    stm_amd.lib().stm_set_agg_variant(variant)
    try:
        dev.d_adcensus_stm(torch.from_numpy(_frame(name).copy()).cuda(), dl, dr, out, p, stages=3)
        torch.cuda.synchronize()
    finally:
        stm_amd.lib().stm_set_agg_variant(0)
    want = _frame_want(name)
    where = (name, variant)
    assert np.array_equal(dl.cpu().numpy(), want["disp_l"]), where
    assert np.array_equal(dr.cpu().numpy(), want["disp_r"]), where
    assert np.array_equal(out.cpu().numpy(), want["interlaced"]), where
