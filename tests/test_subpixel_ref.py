"""Sub-pixel disparity enhancement (Mei et al. 3.4, last step; stm_dc_subpixel and the frame bit 0x200): the numpy float32
statement of the definition in include/stm_hip.h that the GPU tests (test_gpu_subpixel.py) compare against bit for bit, its
behaviour on hand-built volumes, and -- oracle chain plus numpy only -- that it brings the disparity closer to a fractional
ground truth.  No GPU needed."""
import numpy as np
import pytest


def subpixel_ref(cost, disp, zd):
    """The definition, one float32 numpy operation per line of the C statement, in the same order.
    cost: aggregated volume [D][H][W]; disp: [H][W].  Returns the refined copy."""
    cost = np.ascontiguousarray(cost, dtype=np.float32)
    v = np.array(disp, dtype=np.float32, copy=True)
    D = cost.shape[0]
    with np.errstate(all="ignore"):
        ok = (v == np.floor(v)) & (v >= np.float32(1 - zd)) & (v <= np.float32(D - 2 - zd))
        d = np.where(ok, v, np.float32(0)).astype(np.int64) + zd
        d = np.clip(d, 1, max(D - 2, 1))
        if D < 3:
            return v
        cm = np.take_along_axis(cost, (d - 1)[None], 0)[0]
        c0 = np.take_along_axis(cost, d[None], 0)[0]
        cp = np.take_along_axis(cost, (d + 1)[None], 0)[0]
        ok &= np.isfinite(cm) & np.isfinite(c0) & np.isfinite(cp)
        s = cm + cp
        t = c0 + c0
        den = s - t
        ok &= den > np.float32(0)
        num = cm - cp
        den2 = den + den
        off = num / den2
        off = np.fmin(np.fmax(off, np.float32(-0.5)), np.float32(0.5))
        out = v + off
    assert out.dtype == np.float32
    return np.where(ok, out, v)


def oracle_frame(orc, sbs, p, stages, subpixel):
    """The frame pipeline composed from the oracle's stages (d_io.cu order, as orc_adcensus_stm runs it), with the numpy
    sub-pixel step after region voting (stages 2, 3) or on the WTA maps (stage 1).  Returns (disp_l, disp_r, interlaced or
    None).  p: device_api.FrameParams (any object with its fields)."""
    H, Wsbs, _ = sbs.shape
    W = Wsbs // 2
    D, zd = p.num_disp, p.zero_disp
    L, R = orc.demux_sbs(sbs, W)
    cl, cr = orc.ci_adcensus(L, R, p.ad_coeff, p.census_coeff, D, zd)
    xl, al = orc.ca_cross(L, cl, p.ucd, p.lcd, p.usd, p.lsd)
    xr, ar = orc.ca_cross(R, cr, p.ucd, p.lcd, p.usd, p.lsd)
    wl, wr = orc.dc_wta(al, zd), orc.dc_wta(ar, zd)
    if stages == 1:
        if subpixel:
            wl, wr = subpixel_ref(al, wl, zd), subpixel_ref(ar, wr, zd)
        return wl, wr, None
    ol, orr = orc.dr_dcc(wl, wr)
    wl, _ = orc.dr_irv(wl, ol, xl, p.thresh_s, p.thresh_h, D, zd, p.usd, 5, device_flavour=True)
    wr, _ = orc.dr_irv(wr, orr, xr, p.thresh_s, p.thresh_h, D, zd, p.usd, 5, device_flavour=True)
    if subpixel:
        wl, wr = subpixel_ref(al, wl, zd), subpixel_ref(ar, wr, zd)
    dl, dr = orc.filter_bilateral_1(wl, 7, 5.0, 10.0, D), orc.filter_bilateral_1(wr, 7, 5.0, 10.0, D)
    if stages == 2:
        return dl, dr, None
    occl_l, occl_r = orc.dibr_occl(dl, dr)
    occl_l, occl_r = orc.filter_bleed_1(occl_l, 1), orc.filter_bleed_1(occl_r, 1)
    ml, mr = orc.dibr_occl_to_mask(occl_l, occl_r)
    N = p.num_views
    views = [R]
    for v in range(1, N - 1):
        shift = float(np.float32(1.0 - (1.0 * float(np.float32(v))) / (float(np.float32(N)) - 1.0)))
        views.append(orc.dibr_dbm(L, R, dl, dr, ml, mr, shift))
    views.append(L)
    return dl, dr, orc.mux_multiview(views, p.angle, H, W)


class _P:
    """device_api.FrameParams' defaults without importing torch."""

    def __init__(self, num_disp, zero_disp, usd=34, lsd=17):
        self.num_disp, self.zero_disp, self.num_views, self.angle = num_disp, zero_disp, 8, 18.43
        self.ad_coeff, self.census_coeff, self.ucd, self.lcd = 10.0, 30.0, 6.0, 20.0
        self.usd, self.lsd, self.thresh_s, self.thresh_h = usd, lsd, 20, 0.4


# ----------------------------------------------------------------------------- the definition on hand-built volumes
def _column(costs):
    """a [D][1][1] volume from a list of per-hypothesis costs"""
    return np.array(costs, np.float32).reshape(-1, 1, 1)


def test_parabola_vertex_is_found_exactly():
    D, zd = 12, 3
    c = _column([(d - 5.25) ** 2 for d in range(D)])
    out = subpixel_ref(c, np.array([[5 - zd]], np.float32), zd)
    assert out[0, 0] == np.float32(5.25 - zd)
    # and from either neighbour's side the clamp keeps it within half a pixel of the chosen d
    assert subpixel_ref(c, np.array([[6 - zd]], np.float32), zd)[0, 0] == np.float32(6 - zd - 0.5)


@pytest.mark.parametrize("case", ["flat", "concave", "d0", "dlast", "nan_left", "inf_right", "nan_centre", "fraction",
                                  "above_range", "below_range", "nan_disp", "inf_disp"])
def test_ineligible_pixels_are_unchanged(case):
    D, zd = 10, 4
    conv = [(d - 5.3) ** 2 for d in range(D)]
    costs, v = conv, 5.0 - zd
    if case == "flat":
        costs = [7.0] * D
    elif case == "concave":
        costs = [-(d - 5.0) ** 2 for d in range(D)]
    elif case == "d0":
        v = 0.0 - zd
    elif case == "dlast":
        v = float(D - 1 - zd)
    elif case == "nan_left":
        costs = list(conv); costs[4] = np.nan
    elif case == "inf_right":
        costs = list(conv); costs[6] = np.inf
    elif case == "nan_centre":
        costs = list(conv); costs[5] = np.nan
    elif case == "fraction":
        v = 5.5 - zd
    elif case == "above_range":
        v = float(D + 3 - zd)
    elif case == "below_range":
        v = float(-zd - 3)
    elif case == "nan_disp":
        v = np.nan
    elif case == "inf_disp":
        v = np.inf
    disp = np.array([[v]], np.float32)
    out = subpixel_ref(_column(costs), disp, zd)
    assert np.array_equal(out, disp, equal_nan=True), (case, out)


def test_clamp_on_a_voted_d_that_is_not_a_minimum():
    """region voting may hand over a d whose left neighbour costs less: the offset is clamped to -0.5"""
    D, zd = 8, 2
    costs = [9.0, 0.0, 1.0, 3.0, 9.0, 9.0, 9.0, 9.0]  # d = 2: cm 0, c0 1, cp 3 -> den 1, off = -3 / 2 -> -0.5
    out = subpixel_ref(_column(costs), np.array([[2 - zd]], np.float32), zd)
    assert out[0, 0] == np.float32(2 - zd - 0.5)
    costs = [9.0, 3.0, 1.0, 0.0, 9.0, 9.0, 9.0, 9.0]
    assert subpixel_ref(_column(costs), np.array([[2 - zd]], np.float32), zd)[0, 0] == np.float32(2 - zd + 0.5)


def test_reference_is_one_float32_operation_per_step():
    """the vectorised reference against a scalar float32 statement of the same lines, pixel by pixel, on a random volume"""
    rng = np.random.RandomState(5)
    D, H, W, zd = 9, 16, 24, 4
    cost = (rng.rand(D, H, W) * 1000).astype(np.float32)
    disp = (rng.randint(-zd, D - zd, size=(H, W))).astype(np.float32)
    out = subpixel_ref(cost, disp, zd)
    d = disp.astype(np.int64) + zd
    for y in range(H):
        for x in range(W):
            k = d[y, x]
            if not 1 <= k <= D - 2:
                assert out[y, x] == disp[y, x]
                continue
            cm, c0, cp = (np.float32(cost[k + j, y, x]) for j in (-1, 0, 1))
            den = np.float32(np.float32(cm + cp) - np.float32(c0 + c0))
            if not den > 0:
                assert out[y, x] == disp[y, x]
                continue
            off = np.float32(np.float32(cm - cp) / np.float32(den + den))
            off = min(max(off, np.float32(-0.5)), np.float32(0.5))
            assert out[y, x] == np.float32(disp[y, x] + off)


def test_composed_chain_is_the_oracle_frame(orc):
    """oracle_frame without the sub-pixel step is orc_adcensus_stm: the composition the GPU tests use is the frame's"""
    from stm_amd import synth
    H, W, D, zd = 40, 64, 16, 8
    p = _P(D, zd, usd=17, lsd=8)
    sbs, _ = synth.sbs_frame(H, W, D, zd)
    want = orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                            p.thresh_s, p.thresh_h)
    dl, dr, mux = oracle_frame(orc, sbs, p, 3, False)
    assert np.array_equal(dl, want["disp_l"]) and np.array_equal(dr, want["disp_r"])
    assert np.array_equal(mux, want["interlaced"])
    wl, wr, _ = oracle_frame(orc, sbs, p, 1, False)
    assert np.array_equal(wl, want["wta_l"]) and np.array_equal(wr, want["wta_r"])


# ----------------------------------------------------------------------------- quality against a fractional truth
def _slanted_pair(H, W, a, b, seed=3):
    """Left image = a smooth texture T(x, y); right image sampled so that L(x) = R(x + t(x)), t(x) = a + b x (the left
    view's cost pairs L(x) with R(x + (d - zd))).  With t linear, R(x') = T((x' - a) / (1 + b)): a stretched copy."""
    rng = np.random.RandomState(seed)
    yy = np.arange(H, dtype=np.float64)[:, None]

    def texture(u):
        img = np.zeros((H, u.shape[1], 3))
        for c in range(3):
            for _ in range(6):
                fx, fy = rng.uniform(0.05, 0.35), rng.uniform(0.02, 0.2)
                ph = rng.uniform(0, 2 * np.pi)
                img[..., c] += 20.0 * np.sin(fx * u + fy * yy + ph)
        return img

    state = rng.get_state()
    xl = np.arange(W, dtype=np.float64)[None, :] + 0 * yy
    L = texture(xl)
    rng.set_state(state)
    R = texture((np.arange(W, dtype=np.float64)[None, :] + 0 * yy - a) / (1.0 + b))
    to_u8 = lambda img: np.clip(np.rint(img + 128.0), 0, 255).astype(np.uint8)
    truth = (a + b * np.arange(W, dtype=np.float64))[None, :].repeat(H, 0)
    return to_u8(L), to_u8(R), truth


def test_subpixel_brings_the_map_closer_to_a_fractional_slant(orc):
    """96 x 160 pair, disparity ramp t(x) = -2.3 + 0.03 x (about -2.3 .. +2.5, fractional almost everywhere), D = 16,
    zd = 8; mean |disp - t| of the left map over interior pixels (16-pixel margin):
      stage 1 (WTA):                           0.260 whole-pixel, 0.091 with sub-pixel
      stage 2 (DCC, IRV x5, bilateral 7/5/10): 0.149 whole-pixel, 0.062 with sub-pixel"""
    H, W, D, zd = 96, 160, 16, 8
    L, R, truth = _slanted_pair(H, W, -2.3, 0.03)
    sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
    p = _P(D, zd)
    m = 16
    err = {}
    for stages in (1, 2):
        for sp in (False, True):
            dl, _, _ = oracle_frame(orc, sbs, p, stages, sp)
            err[stages, sp] = float(np.mean(np.abs(dl[m:-m, m:-m] - truth[m:-m, m:-m])))
    for stages in (1, 2):
        assert err[stages, True] < err[stages, False], err
    assert err[1, True] < 0.75 * err[1, False], err
