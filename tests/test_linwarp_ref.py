"""Linear sampling of the views' backward warps (stm_dibr_dbm_lin and the frame bit 0x800): the numpy float32 statement of the
definition in include/stm_hip.h that the GPU tests (test_gpu_linwarp.py) compare against bit for bit -- tied to the oracle's
dibr_dbm through its nearest mode -- its known answers, the frame chain composed from the oracle's stages, and that the
fractional fetch brings the synthesised views of a slanted analytic pair closer to the true intermediate views.  No GPU."""
import numpy as np
import pytest

from test_interp_ref import interp_frame
from test_subpixel_ref import _P, _slanted_pair

HSLO, SUBPIXEL, INTERP, LINEAR_WARP = 0x100, 0x200, 0x400, 0x800


def bwarp_ref(img, mask, disp, s, linear):
    """One backward warp (d_dibr_bwarp.cu:5-22), one float32 numpy operation per line of the definition.  linear = False: the
    reference's truncating fetch; linear = True: alu_bilinear_interp at the untruncated clamped coordinate."""
    H, W, _ = img.shape; f = np.float32
    with np.errstate(all="ignore"):
        fx = (np.arange(W, dtype=f)[None, :] + (disp * f(s)).astype(f)).astype(f)
        fx = np.fmin(np.fmax(fx, f(0)), f(W - 1)); yy = np.arange(H)[:, None]
        if not linear:
            v = img[yy, fx.astype(np.int32), :3]
        else:
            x0 = np.floor(fx).astype(np.int32); x1 = np.minimum(x0 + 1, W - 1)
            wx = (fx - x0.astype(f)).astype(f)
            a = (img[yy, x0, :3].astype(f) * (f(1) - wx)[..., None]).astype(f)
            b = (img[yy, x1, :3].astype(f) * wx[..., None]).astype(f)
            v = (a + b).astype(f).astype(np.uint8)
        return (v.astype(f) * mask[..., None]).astype(f).astype(np.uint8)


def dbm_ref(orc, L, R, dl, dr, ml, mr, shift, linear, g_radius=10, g_sigma=15.0, tm=None):
    """dibr_dbm (d_dibr_bwarp.cu:24-70): both warps, the blend G(1 - mask_r), mux_merge_AB with its u8 wrap.  Returns [H][W][3].
    tm: the blend, when the caller has it already (it does not depend on the view)."""
    f = np.float32
    a = bwarp_ref(L, mr, dr, f(-f(shift)), linear)
    b = bwarp_ref(R, ml, dl, f(1.0 - float(f(shift))), linear)
    if tm is None:
        tm = orc.filter_gaussian_1((f(1) - mr).astype(f), g_radius, g_sigma)
    cb = ((f(1) - tm)[..., None] * a.astype(f)).astype(f); ca = (tm[..., None] * b.astype(f)).astype(f)
    return (cb.astype(np.uint8) + ca.astype(np.uint8)).astype(np.uint8)


def linwarp_frame(orc, sbs, p, extra_bits=0, linear=True, out_rows=None, out_cols=None):
    """The full frame composed from the oracle's stages: test_interp_ref.interp_frame up to the filtered maps (extra_bits: 0x100,
    0x200, 0x400 as in the frame's `stages` word), hit maps, bleed and masks from the oracle, dbm_ref per view, the oracle's
    interlacer.  Returns (disp_l, disp_r, interlaced, views)."""
    H, Wsbs, _ = sbs.shape
    W = Wsbs // 2
    dl, dr, _, info = interp_frame(orc, sbs, p, 2, bool(extra_bits & INTERP), subpixel=bool(extra_bits & SUBPIXEL),
                                   hslo=bool(extra_bits & HSLO))
    L, R = info["img_l"], info["img_r"]
    occl_l, occl_r = orc.dibr_occl(dl, dr)
    occl_l, occl_r = orc.filter_bleed_1(occl_l, 1), orc.filter_bleed_1(occl_r, 1)
    ml, mr = orc.dibr_occl_to_mask(occl_l, occl_r)
    tm = orc.filter_gaussian_1((np.float32(1) - mr).astype(np.float32), 10, 15.0)
    N = p.num_views
    views = [R]
    for v in range(1, N - 1):
        shift = float(np.float32(1.0 - (1.0 * float(np.float32(v))) / (float(np.float32(N)) - 1.0)))
        views.append(dbm_ref(orc, L, R, dl, dr, ml, mr, shift, linear, tm=tm))
    views.append(L)
    return dl, dr, orc.mux_multiview(views, p.angle, out_rows or H, out_cols or W), views


# ----------------------------------------------------------------------------- shared inputs
SHAPES = [(9, 37), (1, 5), (6, 1), (20, 300)]  # odd sizes, one row, one column, more than one 256-wide block
SHIFTS = [0.0, 1.0, 0.5, 4.0 / 7.0]


def warp_case(seed, H, W, elem_sz=3):
    """Random images, maps and masks for one dibr_dbm call: fractional maps with whole numbers, NaN and +-inf mixed in (positions
    far outside the row on both sides included), 0 / 1 masks."""
    rng = np.random.RandomState(seed)
    L = rng.randint(0, 256, size=(H, W, elem_sz)).astype(np.uint8)
    R = rng.randint(0, 256, size=(H, W, elem_sz)).astype(np.uint8)
    maps = []
    for _ in range(2):
        d = rng.uniform(-12, 12, size=(H, W)).astype(np.float32)
        r = rng.rand(H, W)
        d = np.where(r < 0.25, np.round(d / 2) * 2, d).astype(np.float32)  # even whole numbers: whole at shift 0.5 too
        d[r > 0.97] = np.nan
        d[(r > 0.94) & (r <= 0.97)] = np.inf
        d[(r > 0.91) & (r <= 0.94)] = -np.inf
        d[(r > 0.88) & (r <= 0.91)] *= 40
        maps.append(d)
    ml = (rng.rand(H, W) < 0.7).astype(np.float32)
    mr = (rng.rand(H, W) < 0.7).astype(np.float32)
    return L, R, maps[0], maps[1], ml, mr


def _row_image(levels, elem_sz=3):
    """[1][W][elem_sz] image: channel c of pixel x holds levels[x] + c (bytes past the third: 200)"""
    g = np.asarray(levels, np.int32)
    img = np.full((1, g.size, elem_sz), 200, np.uint8)
    for c in range(3):
        img[0, :, c] = g + c
    return img


# (name, image levels of one row, disparity row, factor s, the warped row): the definition's corners
NAN = np.nan
EDGE_CASES = [
    ("whole_number", [10, 20, 30, 40], [1, 1, -2, 0], 1.0, [20, 30, 10, 40]),
    ("whole_product", [10, 20, 30, 40], [2, 2, -4, 2], 0.5, [20, 30, 10, 40]),
    ("clamped_at_0", [10, 20, 30, 40], [-0.5, -7.25, -2.5, -1e9], 1.0, [10, 10, 10, 10]),
    ("clamped_at_wmax", [10, 20, 30, 40], [3.5, 2.25, 1.5, 1e9], 1.0, [40, 40, 40, 40]),
    ("half_truncates", [10, 13], [0.5, -0.5], 1.0, [11, 11]),  # 11.5 -> 11: truncation, not rounding
    ("quarter", [0, 100, 200], [0.25, 0.75, -0.25], 1.0, [25, 175, 175]),
    ("nan_samples_column_0", [10, 20, 30, 40], [NAN, NAN, NAN, NAN], 1.0, [10, 10, 10, 10]),
    ("inf", [10, 20, 30, 40], [np.inf, -np.inf, np.inf, -np.inf], 1.0, [40, 10, 40, 10]),
    ("one_column", [77], [0.5], 1.0, [77]),
]
EDGE_IDS = [c[0] for c in EDGE_CASES]


def edge_dbm_inputs(case, elem_sz=3):
    """An EDGE_CASES row as a dibr_dbm call whose result IS the left-sourced warp: shift = 1 (s = -1 for the left image through
    disp_r, s = 0 for the right image), masks 1, so the blend G(1 - mask_r) is 0.  Returns the inputs and the expected [1][W][3]."""
    _, levels, disp, s, want = case
    L = _row_image(levels, elem_sz)
    R = _row_image([255 - v for v in levels], elem_sz)
    dr = (-np.array([disp], np.float32) * np.float32(s)).astype(np.float32)  # disp_r * (-1) = disp * s (s = 1 or 0.5: exact)
    dl = np.full_like(dr, 3.25)
    ones = np.ones_like(dr)
    return (L, R, dl, dr, ones, ones.copy(), 1.0), _row_image(want)[..., :3]


# ----------------------------------------------------------------------------- the scaffolding is the oracle's
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_nearest_mode_is_the_oracles_dibr_dbm(orc, shape):
    H, W = shape
    L, R, dl, dr, ml, mr = warp_case(100 + H, H, W)
    assert np.isnan(dl).any() or H * W < 10
    for shift in SHIFTS:
        for g in ((10, 15.0), (7, 10.0)):
            want = orc.dibr_dbm(L, R, dl, dr, ml, mr, shift, *g)
            assert np.array_equal(dbm_ref(orc, L, R, dl, dr, ml, mr, shift, False, *g), want), (shift, g)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_linear_mode_differs_where_the_coordinate_is_fractional(orc, shape):
    """... and only there: at whole-number disp * s the two fetches agree exactly"""
    H, W = shape
    L, R, dl, dr, ml, mr = warp_case(100 + H, H, W)
    for shift in SHIFTS:
        lin = dbm_ref(orc, L, R, dl, dr, ml, mr, shift, True)
        near = dbm_ref(orc, L, R, dl, dr, ml, mr, shift, False)
        if W > 1 and shift in SHIFTS[2:]:
            assert not np.array_equal(lin, near), shift
        if W == 1:
            assert np.array_equal(lin, near)
    with np.errstate(all="ignore"):
        wl, wr = np.round(dl), np.round(dr)  # NaN and inf stay: they clamp to a whole position in both modes
    for shift in (0.0, 1.0):
        assert np.array_equal(dbm_ref(orc, L, R, wl, wr, ml, mr, shift, True), dbm_ref(orc, L, R, wl, wr, ml, mr, shift, False))


# ----------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_known_answers(orc, case):
    name, levels, disp, s, want = case
    img = _row_image(levels)
    ones = np.ones((1, len(levels)), np.float32)
    got = bwarp_ref(img, ones, np.array([disp], np.float32), s, True)
    assert np.array_equal(got, _row_image(want)), (name, got[0, :, 0])
    if name in ("whole_number", "whole_product", "nan_samples_column_0", "inf", "one_column"):
        assert np.array_equal(bwarp_ref(img, ones, np.array([disp], np.float32), s, False), got)
    args, want_img = edge_dbm_inputs(case)
    assert np.array_equal(dbm_ref(orc, *args, True), want_img), name


def test_mask_scales_the_sample_after_the_truncation():
    img = _row_image([10, 13])
    got = bwarp_ref(img, np.array([[0.5, 0.0]], np.float32), np.array([[0.5, 0.5]], np.float32), 1.0, True)
    assert got[0, :, 0].tolist() == [5, 0]  # (u8)(11 * 0.5), not (u8)(11.5 * 0.5)


# ----------------------------------------------------------------------------- the frame chain
def test_composed_chain_is_the_oracle_frame(orc):
    """linwarp_frame without the linear step is orc_adcensus_stm, also at an output size of its own"""
    from stm_amd import synth
    H, W, D, zd = 40, 64, 16, 8
    p = _P(D, zd, usd=17, lsd=8)
    sbs, _ = synth.sbs_frame(H, W, D, zd)
    for Ho, Wo in ((H, W), (50, 81)):
        want = orc.adcensus_stm(sbs, Ho, Wo, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                                p.thresh_s, p.thresh_h)
        dl, dr, mux, _ = linwarp_frame(orc, sbs, p, 0, linear=False, out_rows=Ho, out_cols=Wo)
        assert np.array_equal(dl, want["disp_l"]) and np.array_equal(dr, want["disp_r"])
        assert np.array_equal(mux, want["interlaced"])
    _, _, lin, _ = linwarp_frame(orc, sbs, p, 0)
    assert lin.shape == (H, W, 3)
    assert not np.array_equal(lin, linwarp_frame(orc, sbs, p, 0, linear=False)[2])


# ----------------------------------------------------------------------------- quality against the true intermediate views
def _true_view(H, W, a, b, t, seed=3):
    """The slanted pair's texture T (test_subpixel_ref._slanted_pair, same generator state) seen from the position `t` between
    the left (t = 0) and the right (t = 1) camera: a left pixel x lands at x + t (a + b x), so view_t(x) = T((x - t a) / (1 + t b))."""
    rng = np.random.RandomState(seed)
    yy = np.arange(H, dtype=np.float64)[:, None]
    u = (np.arange(W, dtype=np.float64)[None, :] + 0 * yy - t * a) / (1.0 + t * b)
    img = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(6):
            fx, fy = rng.uniform(0.05, 0.35), rng.uniform(0.02, 0.2)
            ph = rng.uniform(0, 2 * np.pi)
            img[..., c] += 20.0 * np.sin(fx * u + fy * yy + ph)
    return np.clip(img + 128.0, 0, 255)


@pytest.mark.parametrize("subpixel", [False, True], ids=["whole_pixel_maps", "subpixel_maps"])
def test_linear_sampling_brings_the_views_closer_to_the_truth(orc, subpixel):
    """96 x 160 slanted pair (t(x) = -2.3 + 0.03 x), D = 16, zd = 8, stage-2 maps, views 1 / 3 / 4 / 6 of 8, mean |view - truth|
    over the interior (16-pixel margin), nearest -> linear:
      maps of stages 2:         2.584 / 2.655 / 2.536 / 2.769 -> 0.907 / 0.698 / 0.617 / 0.496
      maps of stages 2 | 0x200: 2.843 / 2.924 / 2.845 / 3.107 -> 0.601 / 0.561 / 0.551 / 0.534
    (the truth left unrounded; against the truth rounded to u8 every figure is a few hundredths lower).  The bound 0.5 leaves room
    for nothing but a bug: the definition itself gives ratios of 0.17 - 0.35."""
    H, W, D, zd, a, b = 96, 160, 16, 8, -2.3, 0.03
    L, R, _ = _slanted_pair(H, W, a, b)
    assert np.array_equal(np.rint(_true_view(H, W, a, b, 0.0)).astype(np.uint8), L)  # the same texture
    assert np.array_equal(np.rint(_true_view(H, W, a, b, 1.0)).astype(np.uint8), R)
    sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
    p = _P(D, zd)
    extra = SUBPIXEL if subpixel else 0
    views_lin = linwarp_frame(orc, sbs, p, extra, linear=True)[3]
    views_near = linwarp_frame(orc, sbs, p, extra, linear=False)[3]
    m = 16
    for v in (1, 3, 4, 6):
        t = 1.0 - v / 7.0  # the view's shift: view 0 = the right image (1), view N - 1 = the left image (0)
        truth = _true_view(H, W, a, b, t)[m:-m, m:-m]
        e_lin = float(np.mean(np.abs(views_lin[v][m:-m, m:-m] - truth)))
        e_near = float(np.mean(np.abs(views_near[v][m:-m, m:-m] - truth)))
        print("view %d, sub-pixel %d: nearest %.3f, linear %.3f" % (v, subpixel, e_near, e_lin))
        assert e_lin < 0.5 * e_near, (v, e_near, e_lin)
