"""Guided disparity up-sampling (stm_disp_upsample and the reduced-resolution frame's bit 0x1000): the numpy float32 statement of
the definition in include/stm_hip.h that the GPU tests (test_gpu_upsample.py) compare against bit for bit -- a vectorised form
and a plain scalar loop, tied to each other pixel by pixel -- its known answers, the reduced-resolution frame composed from the
oracle's stages (tied to the oracle's adcensus_stm_2), and that on a layered scene, whose depth edges are colour edges, the
guided form brings the up-scaled maps closer to the true offsets next to the discontinuities than the bilinear blend.  No GPU."""
import math

import numpy as np
import pytest

from test_interp_ref import interp_frame
from test_linwarp_ref import dbm_ref
from test_subpixel_ref import _P

HSLO, SUBPIXEL, INTERP, LINEAR_WARP, GUIDED_UP = 0x100, 0x200, 0x400, 0x800, 0x1000
SIGMA = 15.0  # the frame's sigma_color
F = np.float32


def up_table(sigma_color):
    """tab[s] = (float)exp(-(double)(s * s) / (2.0 * (double)sigma * (double)sigma)), s = 0 .. 765: the C library's exp, entry by
    entry, rounded once"""
    sg = float(F(sigma_color))
    return np.array([math.exp(-float(s * s) / (2.0 * sg * sg)) for s in range(766)], np.float64).astype(F)


def _src(n_out, n_in):
    """tx_disp_scale's mapping of the output coordinates 0 .. n_out - 1 to the input, one float32 operation at a time"""
    s = ((np.arange(n_out, dtype=F) / F(n_out)).astype(F) * F(n_in)).astype(F)
    return np.fmin(np.fmax(s, F(0)), F(n_in - 1))


def upsample_ref(orc, dlow, ilow, img, up, sigma_color, return_sw=False):
    """The definition on whole arrays, one float32 numpy operation per line of it.  dlow float32 [h][w], ilow uint8 [h][w][>= 3],
    img uint8 [H][W][>= 3].  Returns the [H][W] map (and the weight sums: sw == 0 marks the pixels that took the fallback)."""
    dlow = np.ascontiguousarray(dlow, dtype=F)
    h, w = dlow.shape
    H, W = img.shape[:2]
    assert ilow.shape[:2] == (h, w) and sigma_color > 0
    tab = up_table(sigma_color)
    xs, ys = _src(W, w)[None, :], _src(H, h)[:, None]
    x0, y0 = np.floor(xs).astype(np.int32), np.floor(ys).astype(np.int32)
    g, lo = img[..., :3].astype(np.int32), ilow[..., :3].astype(np.int32)
    sw, swd = np.zeros((H, W), F), np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        for j in (-1, 0, 1, 2):
            yi = y0 + j
            row_in = (yi >= 0) & (yi < h)
            yc = np.clip(yi, 0, h - 1)
            wy = (np.abs((ys - yi.astype(F)).astype(F)) * F(0.5)).astype(F)
            wy = np.fmax(F(0), (F(1) - wy).astype(F))
            for i in (-1, 0, 1, 2):
                xi = x0 + i
                ok = row_in & (xi >= 0) & (xi < w)
                xc = np.clip(xi, 0, w - 1)
                wx = (np.abs((xs - xi.astype(F)).astype(F)) * F(0.5)).astype(F)
                wx = np.fmax(F(0), (F(1) - wx).astype(F))
                sad = np.abs(g - lo[yc, xc]).sum(axis=-1)
                wgt = ((wy * wx).astype(F) * tab[sad]).astype(F)
                t = (wgt * dlow[yc, xc]).astype(F)
                sw = np.where(ok, (sw + wgt).astype(F), sw)
                swd = np.where(ok, (swd + t).astype(F), swd)
        bil = orc.tx_disp_scale(dlow, H, W, 1.0)
        r = np.where(sw > 0, (swd / np.where(sw > 0, sw, F(1))).astype(F), bil)
        out = (r * F(up)).astype(F)
    assert out.dtype == F and sw.dtype == F
    return (out, sw) if return_sw else out


def upsample_loop(orc, dlow, ilow, img, up, sigma_color, taps=None):
    """The definition read aloud: one pixel, one tap, one float32 operation at a time.  taps: an [H][W] int array that receives
    the number of taps that took part."""
    dlow = np.ascontiguousarray(dlow, dtype=F)
    h, w = dlow.shape
    H, W = img.shape[:2]
    tab = up_table(sigma_color)
    bil = orc.tx_disp_scale(dlow, H, W, 1.0)
    out = np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        for y in range(H):
            ys = F(F(F(y) / F(H)) * F(h))
            ys = F(min(max(ys, F(0)), F(h - 1)))
            y0 = int(math.floor(ys))
            for x in range(W):
                xs = F(F(F(x) / F(W)) * F(w))
                xs = F(min(max(xs, F(0)), F(w - 1)))
                x0 = int(math.floor(xs))
                sw, swd, n = F(0), F(0), 0
                for j in (-1, 0, 1, 2):
                    yi = y0 + j
                    if yi < 0 or yi >= h:
                        continue
                    wy = F(max(F(0), F(F(1) - F(abs(F(ys - F(yi))) * F(0.5)))))
                    for i in (-1, 0, 1, 2):
                        xi = x0 + i
                        if xi < 0 or xi >= w:
                            continue
                        wx = F(max(F(0), F(F(1) - F(abs(F(xs - F(xi))) * F(0.5)))))
                        sad = sum(abs(int(img[y, x, c]) - int(ilow[yi, xi, c])) for c in range(3))
                        wgt = F(F(wy * wx) * tab[sad])
                        sw = F(sw + wgt)
                        t = F(wgt * dlow[yi, xi])
                        swd = F(swd + t)
                        n += 1
                r = F(swd / sw) if sw > 0 else bil[y, x]
                out[y, x] = F(r * F(up))
                if taps is not None:
                    taps[y, x] = n
    return out


def render_ref(orc, L, R, dl, dr, p, linear, out_rows, out_cols):
    """hit maps, bleed, masks, N - 2 views, interlacing from full-resolution images and maps: test_linwarp_ref.linwarp_frame's render"""
    occl_l, occl_r = orc.dibr_occl(dl, dr)
    occl_l, occl_r = orc.filter_bleed_1(occl_l, 1), orc.filter_bleed_1(occl_r, 1)
    ml, mr = orc.dibr_occl_to_mask(occl_l, occl_r)
    tm = orc.filter_gaussian_1((F(1) - mr).astype(F), 10, 15.0)
    N = p.num_views
    views = [R]
    for v in range(1, N - 1):
        shift = float(F(1.0 - (1.0 * float(F(v))) / (float(F(N)) - 1.0)))
        views.append(dbm_ref(orc, L, R, dl, dr, ml, mr, shift, linear, tm=tm))
    views.append(L)
    return orc.mux_multiview(views, p.angle, out_rows, out_cols)


def upsample_frame(orc, sbs, p, h, w, disp_scale, extra_bits=0, out_rows=None, out_cols=None, render=True):
    """The reduced-resolution frame composed from the oracle's stages: the split, the bilinear reduction of both views,
    test_interp_ref.interp_frame on the reduced side-by-side frame (extra_bits 0x100 / 0x200 / 0x400), the up-scale by
    up = 1 / disp_scale -- upsample_ref with 0x1000, the oracle's tx_disp_scale without -- and the full-resolution render (linear
    sampling with 0x800).  Returns (disp_l, disp_r, interlaced or None, info)."""
    H, Wsbs, _ = sbs.shape
    W = Wsbs // 2
    L, R = orc.demux_sbs(sbs, W)
    low_l, low_r = orc.tx_scale_bilinear(L, h, w), orc.tx_scale_bilinear(R, h, w)
    low_sbs = np.ascontiguousarray(np.concatenate([low_l, low_r], axis=1))
    ll, lr, _, _ = interp_frame(orc, low_sbs, p, 2, bool(extra_bits & INTERP), subpixel=bool(extra_bits & SUBPIXEL),
                                hslo=bool(extra_bits & HSLO))
    up = float(F(1) / F(disp_scale))
    if extra_bits & GUIDED_UP:
        dl, dr = upsample_ref(orc, ll, low_l, L, up, SIGMA), upsample_ref(orc, lr, low_r, R, up, SIGMA)
    else:
        dl, dr = orc.tx_disp_scale(ll, H, W, up), orc.tx_disp_scale(lr, H, W, up)
    info = {"low_l": ll, "low_r": lr, "img_l": L, "img_r": R, "img_low_l": low_l, "img_low_r": low_r}
    mux = render_ref(orc, L, R, dl, dr, p, bool(extra_bits & LINEAR_WARP), out_rows or H, out_cols or W) if render else None
    return dl, dr, mux, info


# ----------------------------------------------------------------------------- shared inputs
# (H, W) <- (h, w): a non-integer ratio, one row, one column, more than one 256-wide block, ratio 3, ratio 1, a down-scale
SHAPES = [((9, 37), (5, 19)), ((1, 5), (1, 3)), ((6, 1), (3, 1)), ((20, 300), (10, 150)), ((30, 90), (10, 30)), ((7, 11), (7, 11)),
          ((8, 16), (12, 24))]
SHAPE_IDS = ["%dx%d_from_%dx%d" % (s[0] + s[1]) for s in SHAPES]
# ... and reductions strong enough that a block's taps no longer fit its staging buffer at the full tile size: the kernel's
# launcher takes a smaller tile (4 / 3 still fits at 64 x 4; 64 x 4 -> 64 x 2 -> 64 x 1 -> 32 x 1 ...)
STRONG_REDUCTIONS = [((6, 70), (13, 180)), ((5, 66), (40, 400)), ((3, 9), (50, 300))]
PALETTE = np.array([[0, 0, 0], [255, 255, 255], [250, 10, 20], [10, 240, 30], [20, 5, 250]], np.int32)  # pairwise |d| >= 455


def _patches(rng, H, W, cell, elem_sz):
    """flat patches of the palette's colours with a little noise (nearly equal colours: weights in (0, 1))"""
    idx = rng.randint(0, len(PALETTE), size=(H // cell + 1, W // cell + 1))
    img = PALETTE[np.kron(idx, np.ones((cell, cell), np.int64))[:H, :W]]
    img = np.clip(img + rng.randint(-4, 5, size=(H, W, 3)), 0, 255)
    out = rng.randint(0, 256, size=(H, W, elem_sz)).astype(np.uint8)  # bytes past the third: never read
    out[..., :3] = img
    return out


def upsample_case(seed, H, W, h, w, elem_sz=3, nonfinite=True):
    """Guide and low-resolution image in flat patches drawn independently (so some guide pixels meet no tap of their colour:
    sw == 0, and most meet some: sw > 0), a map with NaN, +-inf and large values mixed in.  Returns (dlow, ilow, img)."""
    rng = np.random.RandomState(seed)
    img = _patches(rng, H, W, 4, elem_sz)
    ilow = _patches(rng, h, w, 3, elem_sz)
    d = rng.uniform(-20, 20, size=(h, w)).astype(F)
    r = rng.rand(h, w)
    d[r < 0.2] = np.round(d[r < 0.2])
    if nonfinite:
        d[r > 0.99] = np.nan
        d[(r > 0.98) & (r <= 0.99)] = np.inf
        d[(r > 0.97) & (r <= 0.98)] = -np.inf
        d[(r > 0.94) & (r <= 0.97)] *= F(1e30)
        if d.size >= 12:  # every kind in every map that has room for them
            d.flat[d.size // 5], d.flat[d.size // 2], d.flat[d.size - 2] = np.nan, np.inf, -np.inf
    return d, ilow, img


COL_A, COL_B = (10, 20, 30), (200, 180, 220)  # |d| = 540: tab[540] = exp(-648) is exactly 0


def step_case(elem_sz=3):
    """A two-colour step in a 8 x 16 guide (edge between columns 8 and 9) and in the 4 x 8 low-resolution image (between columns
    4 and 5), the low-resolution map 4 on one side and -2 on the other.  The cross-colour weight is exactly 0 and the values are
    powers of two, so every output pixel is exactly its own side's value times up.  Returns (dlow, ilow, img, up, expected)."""
    H, W, h, w, up = 8, 16, 4, 8, 2.0
    img = np.full((H, W, elem_sz), 77, np.uint8)
    ilow = np.full((h, w, elem_sz), 99, np.uint8)
    img[:, :9, :3], img[:, 9:, :3] = COL_A, COL_B
    ilow[:, :5, :3], ilow[:, 5:, :3] = COL_A, COL_B
    dlow = np.ascontiguousarray(np.broadcast_to(np.where(np.arange(w) < 5, F(4), F(-2)).astype(F), (h, w)))
    want = np.ascontiguousarray(np.broadcast_to(np.where(np.arange(W) < 9, F(8), F(-4)).astype(F), (H, W)))
    return dlow, ilow, img, up, want


def lone_colour_case(elem_sz=3):
    """A flat guide with one pixel of a colour no low-resolution pixel has: that pixel is exactly the bilinear value.
    Returns (dlow, ilow, img, up, (y, x))."""
    rng = np.random.RandomState(5)
    H, W, h, w = 10, 14, 5, 7
    img = np.full((H, W, elem_sz), 60, np.uint8)
    ilow = np.full((h, w, elem_sz), 62, np.uint8)
    img[6, 9, :3] = (255, 0, 255)
    dlow = rng.uniform(-9, 9, size=(h, w)).astype(F)
    return dlow, ilow, img, 2.0, (6, 9)


# ----------------------------------------------------------------------------- the two forms are one definition
@pytest.mark.parametrize("shape", SHAPES + STRONG_REDUCTIONS[:1], ids=SHAPE_IDS + ["6x70_from_13x180"])
def test_vectorised_form_is_the_scalar_loop(orc, shape):
    (H, W), (h, w) = shape
    dlow, ilow, img = upsample_case(H * 7 + w, H, W, h, w, nonfinite=False)
    got, sw = upsample_ref(orc, dlow, ilow, img, 2.0, SIGMA, return_sw=True)
    assert np.isfinite(got).all() and np.isfinite(sw).all()
    assert np.array_equal(got, upsample_loop(orc, dlow, ilow, img, 2.0, SIGMA))


def test_non_finite_maps_follow_the_scalar_loop(orc):
    """NaN and +-inf in the map: an in-image tap takes part whatever its weight (0 * inf = NaN), a skipped tap never does"""
    (H, W), (h, w) = SHAPES[0]
    for elem_sz in (3, 4):
        dlow, ilow, img = upsample_case(3, H, W, h, w, elem_sz)
        assert np.isnan(dlow).any() and np.isposinf(dlow).any() and np.isneginf(dlow).any()
        got, sw = upsample_ref(orc, dlow, ilow, img, 0.5, SIGMA, return_sw=True)
        assert np.isfinite(sw).all()  # the weights never see the map
        assert np.isnan(got).any() and np.isfinite(got).any()
        assert np.array_equal(got, upsample_loop(orc, dlow, ilow, img, 0.5, SIGMA), equal_nan=True)


def test_random_cases_take_both_branches(orc):
    for ((H, W), (h, w)) in SHAPES + STRONG_REDUCTIONS:
        dlow, ilow, img = upsample_case(H * 7 + w, H, W, h, w)
        _, sw = upsample_ref(orc, dlow, ilow, img, 2.0, SIGMA, return_sw=True)
        if H * W >= 60:
            assert (sw == 0).any() and (sw > 0).any(), (H, W)


# ----------------------------------------------------------------------------- known answers
def test_table():
    tab = up_table(SIGMA)
    assert tab[0] == 1 and tab[540] == 0 and tab.dtype == F and len(tab) == 766
    assert tab[15] == F(math.exp(-0.5)) and np.all(np.diff(tab) <= 0)


def test_step_image_keeps_both_sides_exact(orc):
    dlow, ilow, img, up, want = step_case()
    got = upsample_ref(orc, dlow, ilow, img, up, SIGMA)
    assert np.array_equal(got, want), got[0]
    bil = orc.tx_disp_scale(dlow, 8, 16, up)
    assert not np.array_equal(bil, want)  # the bilinear blend invents values between the two surfaces
    assert ((bil > -4) & (bil < 8)).any()


def test_colour_met_by_no_tap_takes_the_bilinear_value(orc):
    dlow, ilow, img, up, (y, x) = lone_colour_case()
    got, sw = upsample_ref(orc, dlow, ilow, img, up, SIGMA, return_sw=True)
    bil = orc.tx_disp_scale(dlow, img.shape[0], img.shape[1], up)
    assert sw[y, x] == 0 and np.count_nonzero(sw == 0) == 1
    assert got[y, x] == bil[y, x]
    assert not np.array_equal(got, bil)  # everywhere else the sixteen taps are not the four


def test_corner_pixels_use_the_taps_inside_the_image_only(orc):
    """8 x 16 <- 4 x 8: the top-left pixel has 3 x 3 taps (row and column -1 skipped), the bottom-right one 2 x 2 (xs clamps to
    w - 1); a NaN just outside a corner's taps does not reach it, an inf under a tap of weight 0 does"""
    H, W, h, w = 8, 16, 4, 8
    img = np.full((H, W, 3), 90, np.uint8)
    ilow = np.full((h, w, 3), 91, np.uint8)
    dlow = np.arange(h * w, dtype=F).reshape(h, w)
    taps = np.zeros((H, W), np.int32)
    base = upsample_loop(orc, dlow, ilow, img, 1.0, SIGMA, taps=taps)
    assert taps[0, 0] == 9 and taps[H - 1, W - 1] == 4 and taps[0, W - 1] == 6 and taps[2, 8] == 16
    assert np.array_equal(base, upsample_ref(orc, dlow, ilow, img, 1.0, SIGMA))
    far = dlow.copy()
    far[0, 3] = np.nan  # column x0 + 3 of pixel (0, 0)
    far[3, 0] = np.nan
    assert upsample_ref(orc, far, ilow, img, 1.0, SIGMA)[0, 0] == base[0, 0]
    zero_weight = dlow.copy()
    zero_weight[0, 2] = np.inf  # xi = x0 + 2 at xs = 0: wx = 1 - 2 * 0.5 = 0, and 0 * inf is NaN
    assert np.isnan(upsample_ref(orc, zero_weight, ilow, img, 1.0, SIGMA)[0, 0])


# ----------------------------------------------------------------------------- the frame chain
FRAMES = [(48, 100, 24, 50, 0), (37, 83, 19, 41, 61)]  # (H, W, h, w, seed offset): ratio 2 and a non-integer ratio


@pytest.mark.parametrize("H,W,h,w,dseed", FRAMES, ids=["48x100", "37x83"])
def test_composed_chain_is_the_oracles_reduced_frame(orc, H, W, h, w, dseed):
    """upsample_frame without extra bits is orc.adcensus_stm_2 element for element, also at an output size of its own"""
    from stm_amd import synth
    D, zd = 16, 8
    p = _P(D, zd, usd=9, lsd=4)
    sbs, _ = synth.sbs_frame(H, W, 2 * D, 2 * zd, seed=synth.SEED + dseed)
    scale = float(w) / float(W)
    for Ho, Wo in ((H, W), (50, 121)):
        want = orc.adcensus_stm_2(sbs, Ho, Wo, h, w, scale, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd,
                                  p.lsd, p.thresh_s, p.thresh_h)
        dl, dr, mux, _ = upsample_frame(orc, sbs, p, h, w, scale, 0, out_rows=Ho, out_cols=Wo)
        assert np.array_equal(dl, want["disp_l"]) and np.array_equal(dr, want["disp_r"])
        assert np.array_equal(mux, want["interlaced"])
    gl, gr, gmux, _ = upsample_frame(orc, sbs, p, h, w, scale, GUIDED_UP)
    assert gl.shape == (H, W) and not np.array_equal(gr, dr)  # (the first frame's left map is one value: nothing to sharpen)
    assert np.array_equal(gl, dl) == (np.unique(dl).size == 1)
    assert not np.array_equal(gmux, upsample_frame(orc, sbs, p, h, w, scale, 0)[2])


# ----------------------------------------------------------------------------- quality against the true offsets
def layered_scene(H, W, D, zd, seed=0):
    """A scene whose depth edges are colour edges (synth's frames are one continuous texture: theirs are not): the synth texture,
    seven rectangles of 15 - 35 % of H by 10 - 30 % of W, each at an even offset of its own and recoloured L // 2 + 64 + tint (tint
    uniform in -70 .. 70 per channel), the background at the farthest offset.  D, zd: the range of the match at HALF size; the
    full-resolution offsets are twice its offsets.  Returns (sbs, off)."""
    from stm_amd import synth
    rng = np.random.RandomState(1000 + seed)
    L = synth.left_image(H, W, synth.SEED + 900 + seed).astype(np.int32)
    lo, hi = -(zd - 1) + 2, (D - zd - 1) - 2  # synth.disparity_field's margins, at half size
    off = np.full((H, W), 2 * hi, np.int32)
    for _ in range(7):
        rh, rw = int(H * rng.uniform(0.15, 0.35)), int(W * rng.uniform(0.10, 0.30))
        y0, x0 = rng.randint(0, H - rh), rng.randint(0, W - rw)
        off[y0:y0 + rh, x0:x0 + rw] = 2 * rng.randint(lo, hi)  # nearer than the background
        tint = rng.randint(-70, 71, size=3)
        L[y0:y0 + rh, x0:x0 + rw] = L[y0:y0 + rh, x0:x0 + rw] // 2 + 64 + tint
    L = np.clip(L, 0, 255).astype(np.uint8)
    R = synth.right_image(L, off)
    return np.ascontiguousarray(np.concatenate([L, R], axis=1)), off


def edge_band(off, r=4):
    """pixels within r px (Chebyshev) of a discontinuity of the offsets: both pixels of every differing 4-neighbour pair, dilated"""
    H, W = off.shape
    e = np.zeros((H, W), bool)
    dx, dy = off[:, 1:] != off[:, :-1], off[1:] != off[:-1]
    e[:, 1:] |= dx; e[:, :-1] |= dx; e[1:] |= dy; e[:-1] |= dy
    pad = np.pad(e, r - 1)  # the marked pixels are at distance 1 already
    band = np.zeros((H, W), bool)
    for sy in range(2 * r - 1):
        for sx in range(2 * r - 1):
            band |= pad[sy:sy + H, sx:sx + W]
    return band


QUALITY = [("96x160_d16", 96, 160, 16, 8, 0), ("136x240_d16", 136, 240, 16, 8, 1), ("192x320_d24", 192, 320, 24, 12, 2)]


@pytest.mark.parametrize("case", QUALITY[:2], ids=[c[0] for c in QUALITY[:2]])
def test_guided_upsampling_of_the_true_half_resolution_maps(orc, case):
    """The up-sampler alone: fed off[::2, ::2] / 2, mean |disp - truth| over the band, bilinear -> guided (sigma 15):
      96 x 160: 0.761 -> 0.119;  136 x 240: 0.945 -> 0.018   (fallback share 0.000 on both).
    What remains sits on the one or two rectangle borders whose tint leaves little contrast against what lies behind (305 pixels
    carry 92 % of the first figure): with no colour edge there is nothing to be guided by.  Sigma 8 / 30 / 60 give 0.026 / 0.273 /
    0.669 and 0.001 / 0.190 / 0.848.  The bound of a quarter of the bilinear error is the one the feature was specified with."""
    name, H, W, D, zd, seed = case
    sbs, off = layered_scene(H, W, D, zd, seed)
    L = np.ascontiguousarray(sbs[:, :W])
    low = orc.tx_scale_bilinear(L, H // 2, W // 2)
    half = (off[::2, ::2].astype(F) / F(2)).astype(F)
    band = edge_band(off)
    assert band.mean() > 0.1
    bil = orc.tx_disp_scale(half, H, W, 2.0)
    gui, sw = upsample_ref(orc, half, low, L, 2.0, SIGMA, return_sw=True)
    e_bil, e_gui = float(np.abs(bil - off)[band].mean()), float(np.abs(gui - off)[band].mean())
    print("%s true maps: band %.3f of the image, bilinear %.3f, guided %.3f, fallback share %.4f" % (name, band.mean(), e_bil, e_gui,
                                                                                                    (sw == 0).mean()))
    assert e_gui < 0.25 * e_bil, (e_bil, e_gui)


@pytest.mark.parametrize("case", QUALITY, ids=[c[0] for c in QUALITY])
def test_guided_upsampling_of_the_pipelines_own_maps(orc, case):
    """The oracle's stages-2 chain at half size (usd 9, lsd 4), left view, mean |disp - truth| band / whole map (share of band
    pixels off by more than 1 px), bilinear -> guided; direction only is asserted: what remains is the matcher's error in the
    occluded strips, which an up-sampler cannot repair.  Figures: DESIGN.md section 12."""
    name, H, W, D, zd, seed = case
    sbs, off = layered_scene(H, W, D, zd, seed)
    p = _P(D, zd, usd=9, lsd=4)
    band = edge_band(off)
    for extra in (0, INTERP):
        bil = upsample_frame(orc, sbs, p, H // 2, W // 2, 0.5, extra, render=False)[0]
        gui = upsample_frame(orc, sbs, p, H // 2, W // 2, 0.5, extra | GUIDED_UP, render=False)[0]
        eb, eg = np.abs(bil - off), np.abs(gui - off)
        print("%s chain, extra 0x%x: bilinear %.3f / %.3f (%.3f), guided %.3f / %.3f (%.3f)" % (
            name, extra, eb[band].mean(), eb.mean(), (eb[band] > 1).mean(), eg[band].mean(), eg.mean(), (eg[band] > 1).mean()))
        if extra == 0:
            assert eg[band].mean() < eb[band].mean(), (eb[band].mean(), eg[band].mean())
