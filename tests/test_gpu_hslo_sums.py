"""The scanline passes (csrc/stm_kernels_hslo.hip) compared with the CPU oracle on their PATH-COST SUMS, both views.

Every other scanline test compares the winner-takes-all map, which a wrong neighbour at a 64-lane border, a penalty from the wrong
table slot or a `+ m` for a `- m` moves sums under without moving most minima.  Here every case runs stm_d_dc_hslo_view with the test
tap of include/stm_hslo_tap.h set and compares, float for float (np.array_equal: the arithmetic order is the definition, no tolerance
applies), the accumulator behind the horizontal passes (s2 = C_lr + C_rl), behind the top-to-bottom pass (s3) and the final volume the
bottom-to-top kernel forms in registers (fin), and the map -- for the left view (osign +1) and for the right view (osign -1, which no
stage reached before) -- then repeats the call with the tap clear and requires the same map.

The kernel forms: D <= 64 walks a row from both ends in one launch (stm_k_hslo_h2: "h2") or, under stm_set_agg_variant(400), in one
launch per direction (stm_k_hslo_h<1, *, 8>: "h1"); D <= 128 and D <= 256 keep two and four hypotheses per lane ("dpl2", "dpl4":
stm_k_hslo_h<2, *, 4>, <4, *, 2>, with the lane-0 / lane-63 border patches).  The vertical kernels are stm_k_hslo_v<1, *, 8>, <2, *, 4>,
<4, *, 2>.  A row is walked in groups of four pixels, G = ceil(W / 4), each form some groups (rows) ahead: its prefetch depth.

Inputs are finite and every buffer is fully sized; the tap buffers start as NaN, so an element the kernels leave out shows.

One departure from "every case asserts the class-pair condition": hslo_cases.assert_all_class_pairs (all nine (class D1, class D2)
pairs, >= 8 times, in each of the four directions) is asserted by every T = 15 case whose shape can hold it, on palette images that
meet it for both views (hslo_cases.covering_images).  The walk-geometry cases below 8 x 29 cannot -- W = 1 or H = 1 has no step at
all in one orientation -- and are about G and H around the prefetch depths.  The frame runs on palette content, where the condition
is asserted per view, and on the project's synthetic stereo frame as the frame tests before it, whose smooth surfaces hold no step
of exactly 15."""
import numpy as np
import pytest

import hslo_cases as hc

pytestmark = pytest.mark.gpu

FORMS = hc.FORMS  # stm_set_agg_variant's word of the form
VIEWS = [0, 1]
FRAME = hc.PARAM_SETS["frame_15_1_3"]
_ORACLE = {}


def _form_of(D, variant):
    return ("h1" if variant == 400 else "h2") if D <= 64 else "dpl2" if D <= 128 else "dpl4"


def _want(orc, key, cost, own, other, params, zd, view):
    """the oracle's (map, s2, s3, fin) of a case, computed once, read only, and finite"""
    key = key + (view,)
    if key not in _ORACLE:
        res = orc.dc_hslo_sums(cost, own, other, params[0], params[1], params[2], zd, -1 if view else 1)
        for a in res:
            assert np.isfinite(a).all()
            a.setflags(write=False)
        _ORACLE[key] = res
    return _ORACLE[key]


def _gpu(cost, own, other, params, zd, view, variant=0, tap=True):
    """(map, s2, s3, fin) from stm_d_dc_hslo_view under the variant; the three sums are None with the tap clear"""
    import torch
    import stm_amd
    from stm_amd import device_api as dev
    D, H, W = cost.shape
    slab = torch.from_numpy(np.ascontiguousarray(cost)).cuda()
    tab = dev.plane_table(slab)
    t_own, t_other = torch.from_numpy(np.ascontiguousarray(own)).cuda(), torch.from_numpy(np.ascontiguousarray(other)).cuda()
    disp = torch.full((H, W), float("nan"), dtype=torch.float32, device="cuda")
    bufs = [torch.full((1, D, H, W), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)] if tap else [None] * 3
    stm_amd.lib().stm_set_agg_variant(variant)
    try:
        dev.set_hslo_tap(*bufs)
        dev.d_dc_hslo_view(tab, disp, t_own, t_other, params[0], params[1], params[2], D, zd, view)
        torch.cuda.synchronize()
    finally:
        dev.set_hslo_tap()
        stm_amd.lib().stm_set_agg_variant(0)
    return (disp.cpu().numpy(),) + tuple(None if b is None else b[0].cpu().numpy() for b in bufs)


def _check(orc, key, cost, own, other, params, zd, view, variant=0, cover=True):
    if params[0] == 15.0 and cover:
        hc.assert_all_class_pairs(own, other, cost.shape[0], zd, -1 if view else 1, 15.0)
    want = _want(orc, key, cost, own, other, params, zd, view)
    got = _gpu(cost, own, other, params, zd, view, variant)
    for name, g, w in zip(("s2", "s3", "fin", "map"), got[1:] + got[:1], want[1:] + want[:1]):
        bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
        assert np.array_equal(g, w), "%s differs at %d of %d, first at %s: %r for %r" % (
            name, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])
    clear = _gpu(cost, own, other, params, zd, view, variant, tap=False)
    assert np.array_equal(clear[0], want[0])  # the tap changes no result
    return got


def _images(H, W, seed, elem_sz=3):
    return hc.palette_image(H, W, seed, elem_sz), hc.palette_image(H, W, seed + 1000, elem_sz)


_COVERING = {}


def _covering(H, W, D, zd, seed, elem_sz=3):
    """palette images that meet the class-pair condition for both views (hslo_cases.covering_images), found once per shape"""
    key = (H, W, D, zd, seed, elem_sz)
    if key not in _COVERING:
        _COVERING[key] = hc.covering_images(H, W, D, zd, seed, elem_sz)
    return _COVERING[key]


# ----------------------------------------------------------------------------- the forms
# (H, W, D, zd): D <= 64 (both horizontal forms), 65 / 100 / 128 (two per lane), 129 / 200 / 256 (four per lane)
FORM_SHAPES = [(9, 33, 5, 2), (5, 17, 16, 0), (8, 36, 64, 63), (5, 17, 65, 64), (9, 33, 100, 40), (5, 38, 128, 0), (5, 17, 129, 3),
               (9, 33, 200, 90), (5, 33, 256, 255)]


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("variant", [0, 400])
@pytest.mark.parametrize("H,W,D,zd", FORM_SHAPES)
def test_forms(gpu_ready, orc, H, W, D, zd, variant, view):
    """each form on its sums; variant 400 gives the four arrays of the default (both equal the oracle's, and each other), and takes
    the one-launch-per-direction kernels exactly where D <= 64"""
    from stm_amd import device_api as dev
    own, other = _covering(H, W, D, zd, 100 + D)
    cost = hc.cost_volume("uniform", D, H, W, D)
    key = ("forms", H, W, D, zd)
    dev.prof_reset()
    dev.prof_enable(True)
    try:
        got = _check(orc, key, cost, own, other, FRAME, zd, view, variant)
    finally:
        dev.prof_enable(False)
    n_rl = dev.prof_read("hslo_rl")[0]
    assert (n_rl > 0) == (_form_of(D, variant) != "h2"), "hslo_rl launches: %d under variant %d at D = %d" % (n_rl, variant, D)
    if variant == 400:
        default = _gpu(cost, own, other, FRAME, zd, view, 0)
        for a, b in zip(got, default):
            assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- walk geometry
# W -> G: 1, 3, 4 -> 1;  5 -> 2;  9 -> 3;  13 -> 4;  17 -> 5;  29 -> 8;  33, 36 -> 9;  38 -> 10: G = 1, and G below / equal to / one above
# the prefetch depth of each form (h2: 4, h1: 8, dpl2: 4, dpl4: 2), odd and even G for the two-ended handover in the middle of the
# row, and (W % 4 != 0) a last group partly outside the image, the first group the right-to-left walk enters.  9 and 29 are added
# to the widths the forms were asked at, for G = 3 (one above dpl4's depth) and G = 8 (h1's depth itself).
# H around the vertical kernels' prefetch depths 8, 4, 2.  Each W once per form, the heights dealt round.
GEO, GEO_D = hc.GEO, hc.GEO_D  # (tests/test_hslo_cases.py checks without a GPU that every width and height occurs per form)


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("form,H,W", GEO)
def test_walk_geometry(gpu_ready, orc, form, H, W, view):
    """the class-pair condition is asserted where the shape can hold it (hslo_cases.geo_can_cover: H >= 8 and W >= 29); a single row
    or column has no step in one orientation, and the smaller shapes are about the walks' bookkeeping"""
    D, zd = GEO_D[form]
    cover = hc.geo_can_cover(H, W)
    own, other = _covering(H, W, D, zd, 200 + 7 * H + W) if cover else _images(H, W, 200 + 7 * H + W)
    cost = hc.cost_volume("uniform", D, H, W, 31 * H + W)
    _check(orc, ("geo", H, W, D, zd), cost, own, other, FRAME, zd, view, FORMS[form], cover=cover)


# ----------------------------------------------------------------------------- zero_disp
# 0, D - 1 and one between: PAD = max(zd, D - 1 - zd) comes from either side; W = 17 < D in every form: most matched pixels are clamped
ZD_SHAPES = {"h2": (5, 17, 24), "h1": (5, 17, 24), "dpl2": (5, 17, 70), "dpl4": (5, 17, 140)}


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("where", ["zero", "last", "between"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_zero_disp(gpu_ready, orc, form, where, view):
    H, W, D = ZD_SHAPES[form]
    zd = {"zero": 0, "last": D - 1, "between": D // 3}[where]
    own, other = _covering(H, W, D, zd, 300 + D)
    cost = hc.cost_volume("uniform", D, H, W, 3 * D)
    _check(orc, ("zd", H, W, D, zd), cost, own, other, FRAME, zd, view, FORMS[form])


# ----------------------------------------------------------------------------- class planes
@pytest.mark.parametrize("view", VIEWS)
def test_class_planes_wider_than_two_blocks(gpu_ready, orc, view):
    """WP = 4 G + 2 PAD + 8 > 512: stm_k_hslo_classes runs three blocks per row"""
    H, W, D, zd = 3, 520, 12, 5
    own, other = _covering(H, W, D, zd, 400)
    _check(orc, ("wide", H, W, D, zd), hc.cost_volume("uniform", D, H, W, 4), own, other, FRAME, zd, view)


@pytest.mark.parametrize("view", VIEWS)
def test_four_byte_pixels(gpu_ready, orc, view):
    """elem_sz 4: the means read B, G, R of a four-byte pixel and never its fourth byte (random here)"""
    H, W, D, zd = 9, 33, 16, 3
    own, other = _covering(H, W, D, zd, 410, elem_sz=4)
    _check(orc, ("e4", H, W, D, zd), hc.cost_volume("uniform", D, H, W, 5), own, other, FRAME, zd, view)
    # and the fourth byte is indeed ignored: the oracle gives the same sums on the three-byte image
    want3 = orc.dc_hslo_sums(hc.cost_volume("uniform", D, H, W, 5), own[..., :3], other[..., :3], *FRAME, zd, -1 if view else 1)
    assert all(np.array_equal(a, b) for a, b in zip(want3, _ORACLE[("e4", H, W, D, zd, view)]))


# ----------------------------------------------------------------------------- penalties and threshold
PENALTY_SHAPES = {"h2": (9, 33, 5, 2), "dpl2": (5, 17, 70, 30)}


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("form", sorted(PENALTY_SHAPES))
@pytest.mark.parametrize("params", sorted(hc.PARAM_SETS))
def test_penalties_and_threshold(gpu_ready, orc, params, form, view):
    """every (T, H1, H2) of hslo_cases.PARAM_SETS: H / 4 and H / 10 divided in double and narrowed, the '<' / '>' / neither class rule,
    and for T = float32(1/3), on images of unit steps, the float32 rounding of the other image's mean"""
    H, W, D, zd = PENALTY_SHAPES[form]
    p = hc.PARAM_SETS[params]
    if params == "t_one_third":
        own, other = hc.unit_step_image(H, W, 500), hc.unit_step_image(H, W, 501)
        n = hc.class_counts(own, other, D, zd, -1 if view else 1, p[0])
        assert n[:, :2, :2].min() > 0  # D1 and D2 each fall on both sides of T, in every direction
    else:
        own, other = _covering(H, W, D, zd, 510)
    _check(orc, ("pen", params, H, W, D, zd), hc.cost_volume("uniform", D, H, W, 6), own, other, p, zd, view)


# ----------------------------------------------------------------------------- costs
COST_SHAPES = {"h2": (5, 17, 64, 20), "dpl2": (5, 17, 128, 100), "dpl4": (5, 17, 200, 64)}


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("form", sorted(COST_SHAPES))
@pytest.mark.parametrize("kind", ["uniform", "quarters", "constant", "scaled", "planted"])
def test_costs(gpu_ready, orc, kind, form, view):
    """hslo_cases.cost_volume: exact ties, a constant volume (every map value -zero_disp; the cross-lane tie path of WTA at D > 64),
    large values, and minima planted at d = 0, 63, 64, 127, 128 and D - 1"""
    H, W, D, zd = COST_SHAPES[form]
    own, other = _covering(H, W, D, zd, 600 + D)
    got = _check(orc, ("cost", kind, H, W, D, zd), hc.cost_volume(kind, D, H, W, 7), own, other, FRAME, zd, view)
    if kind == "constant":
        assert np.array_equal(got[0], np.full((H, W), -zd, np.float32))


# ----------------------------------------------------------------------------- the frame
@pytest.mark.parametrize("variant", [0, 10000])
@pytest.mark.parametrize("content,H,W,D,zd", [("synth", 37, 203, 20, 7), ("synth", 21, 75, 70, 30), ("palette", 37, 203, 20, 7)])
def test_frame(gpu_ready, orc, content, H, W, D, zd, variant):
    """d_adcensus_stm(stages = 3 | 0x100) with two-view tap buffers: variant 0 runs the passes on the PQ volumes as the aggregation left
    them, columns past W included; 10000 converts them first.  Per view the three sums equal dc_hslo_sums on the oracle's own
    aggregated volumes (built as ref_cases._disp_pair builds them), and the maps and the frame equal the oracle's as before.
    Content: the synthetic stereo frame of the other frame tests, and a pair of palette images (hslo_cases)."""
    import torch
    import stm_amd
    from stm_amd import device_api as dev, synth
    if content == "palette":  # the two eyes are palette images: every penalty class pair in every direction, asserted per view
        pl, pr = _covering(H, W, D, zd, 700)
        hc.assert_all_class_pairs(pl, pr, D, zd, 1)
        hc.assert_all_class_pairs(pr, pl, D, zd, -1)
        sbs = np.ascontiguousarray(np.concatenate([pl, pr], axis=1))
    else:
        sbs, _ = synth.sbs_frame(H, W, D, zd)
    p = dev.FrameParams(num_disp=D, zero_disp=zd, usd=11, lsd=5)
    key = ("frame", content, H, W, D, zd)
    if key not in _ORACLE:
        L, R = np.ascontiguousarray(sbs[:, :W]), np.ascontiguousarray(sbs[:, W:2 * W])
        cl, cr = orc.ci_adcensus(L, R, p.ad_coeff, p.census_coeff, D, zd)
        al, ar = orc.ca_cross(L, cl, p.ucd, p.lcd, p.usd, p.lsd)[1], orc.ca_cross(R, cr, p.ucd, p.lcd, p.usd, p.lsd)[1]
        views = [orc.dc_hslo_sums(al, L, R, *FRAME, zd, 1), orc.dc_hslo_sums(ar, R, L, *FRAME, zd, -1)]
        assert all(np.isfinite(a).all() for v in views for a in v)
        frame = orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                                 p.thresh_s, p.thresh_h, hslo=True)
        wta = orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                               p.thresh_s, p.thresh_h, stop_after_wta=True, hslo=True)
        assert np.array_equal(wta["wta_l"], views[0][0]) and np.array_equal(wta["wta_r"], views[1][0])  # the frame's chain is this chain
        _ORACLE[key] = (views, frame)
    views, frame = _ORACLE[key]
    d_sbs = torch.from_numpy(sbs).cuda()
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    bufs = [torch.full((2, D, H, W), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    stm_amd.lib().stm_set_agg_variant(variant)
    try:
        with dev.hslo_tap(*bufs):
            dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=3 | 0x100)
            torch.cuda.synchronize()
        tapped = dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()
        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=3 | 0x100)  # the tap clear
        torch.cuda.synchronize()
    finally:
        dev.set_hslo_tap()
        stm_amd.lib().stm_set_agg_variant(0)
    for v in (0, 1):
        for k, name in enumerate(("s2", "s3", "fin")):
            assert np.array_equal(bufs[k][v].cpu().numpy(), views[v][1 + k]), "%s of view %d" % (name, v)
    for got in (tapped, (dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy())):
        assert np.array_equal(got[0], frame["disp_l"]) and np.array_equal(got[1], frame["disp_r"])
        assert np.array_equal(got[2], frame["interlaced"])
