"""Outlier interpolation (Mei et al. 3.4, the step after region voting; stm_dr_interp and the frame bit 0x400): the numpy
statement of the definition in include/stm_hip.h that the GPU tests (test_gpu_interp.py) compare against bit for bit -- a
scalar form, the definition read aloud, and a vectorised form tied to it pixel by pixel -- its known answers, the frame chain
composed from the oracle's stages, and that it brings the pixels region voting leaves closer to the true offsets.  No GPU."""
import numpy as np
import pytest

from test_subpixel_ref import _P, subpixel_ref

DIRS = [(1, 0), (2, 1), (1, 1), (1, 2), (0, 1), (-1, 2), (-1, 1), (-2, 1), (-1, 0), (-2, -1), (-1, -1), (-1, -2), (0, -1), (1, -2),
        (1, -1), (2, -1)]


def interp_ref(disp, outl, img):
    """The definition, one pixel and one direction at a time.  disp float32 [H][W], outl uint8 [H][W], img uint8 [H][W][>= 3]."""
    H, W = disp.shape
    out = disp.copy()
    im = img[..., :3].astype(np.int32)
    for y, x in zip(*np.nonzero(outl)):
        occ = outl[y, x] == 2
        have, best, bestc = False, None, None
        for dx, dy in DIRS:
            qx, qy = x + dx, y + dy
            while 0 <= qx < W and 0 <= qy < H:
                if outl[qy, qx] == 0:
                    v = disp[qy, qx]
                    if occ:
                        if not have or v > best:
                            have, best = True, v
                    else:
                        c = int(np.abs(im[qy, qx] - im[y, x]).sum())
                        if not have or c < bestc:
                            have, best, bestc = True, v, c
                    break
                qx += dx
                qy += dy
        if have:
            out[y, x] = best
    return out


def _first_reliable(outl, dx, dy):
    """[H][W] flat index of the first reliable pixel at p + k (dx, dy), k >= 1, or -1: nxt[p] = q if q is reliable else nxt[q],
    q = p + (dx, dy), filled a row (or, for the horizontal directions, a column) at a time, q's before p's."""
    H, W = outl.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    rel = outl == 0
    nxt = np.full((H, W), -1, np.int64)
    if dy != 0:
        xq = np.arange(W) + dx
        ok = (xq >= 0) & (xq < W)
        xc = np.clip(xq, 0, W - 1)
        for y in (range(H - 1, -1, -1) if dy > 0 else range(H)):
            yq = y + dy
            if 0 <= yq < H:
                nxt[y] = np.where(ok, np.where(rel[yq, xc], idx[yq, xc], nxt[yq, xc]), -1)
    else:
        for x in (range(W - 1, -1, -1) if dx > 0 else range(W)):
            xq = x + dx
            if 0 <= xq < W:
                nxt[:, x] = np.where(rel[:, xq], idx[:, xq], nxt[:, xq])
    return nxt


def interp_ref_fast(disp, outl, img):
    """interp_ref with the walks as 16 first-reliable-pixel tables and the fold over the directions, in the definition's order,
    on whole arrays.  test_fast_form_is_the_scalar_form ties it to interp_ref pixel by pixel."""
    disp = np.ascontiguousarray(disp, dtype=np.float32)
    H, W = disp.shape
    im = img[..., :3].astype(np.int32).reshape(H * W, 3)
    flat = disp.reshape(-1)
    todo = outl != 0
    occ = outl == 2
    have = np.zeros((H, W), bool)
    best = disp.copy()
    bestc = np.zeros((H, W), np.int64)
    own = im.reshape(H, W, 3)
    with np.errstate(invalid="ignore"):
        for dx, dy in DIRS:
            c = _first_reliable(outl, dx, dy)
            has = todo & (c >= 0)
            cc = np.maximum(c, 0)
            v = flat[cc]
            cost = np.abs(im[cc] - own).sum(axis=-1)
            take = has & (~have | np.where(occ, v > best, cost < bestc))
            best = np.where(take, v, best)
            bestc = np.where(take, cost, bestc)
            have |= has
    assert best.dtype == np.float32
    return np.where(have, best, disp)


def interp_frame(orc, sbs, p, stages, interp, subpixel=False, hslo=False):
    """The frame pipeline composed from the oracle's stages (as test_subpixel_ref.oracle_frame composes it), stages 2 or 3, with
    the numpy interpolation after region voting and the numpy sub-pixel step after that.  hslo: the chain starts from the
    oracle's post-HSLO maps (orc.adcensus_stm(..., hslo=True)["wta_l" / "wta_r"]) and the arms of orc.ca_cross.
    Returns (disp_l, disp_r, interlaced or None, info); info holds the left view's maps around the step."""
    assert stages in (2, 3)
    H, Wsbs, _ = sbs.shape
    W = Wsbs // 2
    D, zd = p.num_disp, p.zero_disp
    L, R = orc.demux_sbs(sbs, W)
    cl, cr = orc.ci_adcensus(L, R, p.ad_coeff, p.census_coeff, D, zd)
    xl, al = orc.ca_cross(L, cl, p.ucd, p.lcd, p.usd, p.lsd)
    xr, ar = orc.ca_cross(R, cr, p.ucd, p.lcd, p.usd, p.lsd)
    if hslo:
        f = orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                             p.thresh_s, p.thresh_h, hslo=True)
        wl, wr = f["wta_l"], f["wta_r"]
    else:
        wl, wr = orc.dc_wta(al, zd), orc.dc_wta(ar, zd)
    ol, orr = orc.dr_dcc(wl, wr)
    info = {"dcc_l": ol, "dcc_r": orr}
    wl, ol = orc.dr_irv(wl, ol, xl, p.thresh_s, p.thresh_h, D, zd, p.usd, 5, device_flavour=True)
    wr, orr = orc.dr_irv(wr, orr, xr, p.thresh_s, p.thresh_h, D, zd, p.usd, 5, device_flavour=True)
    info.update(voted_l=wl, voted_r=wr, outl_l=ol, outl_r=orr, img_l=L, img_r=R)
    if interp:
        wl, wr = interp_ref_fast(wl, ol, L), interp_ref_fast(wr, orr, R)
    info.update(interp_l=wl, interp_r=wr)
    if subpixel:
        wl, wr = subpixel_ref(al, wl, zd), subpixel_ref(ar, wr, zd)
    dl, dr = orc.filter_bilateral_1(wl, 7, 5.0, 10.0, D), orc.filter_bilateral_1(wr, 7, 5.0, 10.0, D)
    if stages == 2:
        return dl, dr, None, info
    occl_l, occl_r = orc.dibr_occl(dl, dr)
    occl_l, occl_r = orc.filter_bleed_1(occl_l, 1), orc.filter_bleed_1(occl_r, 1)
    ml, mr = orc.dibr_occl_to_mask(occl_l, occl_r)
    N = p.num_views
    views = [R]
    for v in range(1, N - 1):
        shift = float(np.float32(1.0 - (1.0 * float(np.float32(v))) / (float(np.float32(N)) - 1.0)))
        views.append(orc.dibr_dbm(L, R, dl, dr, ml, mr, shift))
    views.append(L)
    return dl, dr, orc.mux_multiview(views, p.angle, H, W), info


def grey(levels):
    """[..., 3] uint8 image, the three channels equal"""
    g = np.asarray(levels, np.uint8)
    return np.ascontiguousarray(np.stack([g, g, g], axis=-1))


def random_case(seed, H, W, elem_sz=3, p_out=0.35):
    """A random map with all of the classes 0, 1, 2 and a stray 7, some NaN and non-integer values, and an image of three grey
    levels (many exact colour ties, so the direction order decides) with a little colour noise in one channel."""
    rng = np.random.RandomState(seed)
    disp = rng.randint(-9, 10, size=(H, W)).astype(np.float32)
    disp[rng.rand(H, W) < 0.08] += np.float32(0.25)
    disp[rng.rand(H, W) < 0.06] = np.nan
    outl = np.zeros((H, W), np.uint8)
    r = rng.rand(H, W)
    outl[r < p_out] = 1
    outl[r < p_out * 0.55] = 2
    outl[r < p_out * 0.08] = 7
    img = np.zeros((H, W, elem_sz), np.uint8)
    img[..., :] = (rng.randint(0, 3, size=(H, W)) * 40 + 60).astype(np.uint8)[..., None]
    noisy = rng.rand(H, W) < 0.2
    img[..., 1] = np.where(noisy, img[..., 1] + rng.randint(0, 3, size=(H, W)), img[..., 1]).astype(np.uint8)
    if elem_sz > 3:
        img[..., 3:] = rng.randint(0, 256, size=(H, W, elem_sz - 3))  # never read
    return disp, outl, img


# (seed, H, W, elem_sz, outlier share): widths that are not a multiple of 64, one row, one column, four bytes per pixel
RANDOM_CASES = [(1, 23, 37, 3, 0.35), (2, 9, 131, 3, 0.6), (3, 1, 75, 3, 0.4), (4, 61, 1, 3, 0.4), (5, 17, 70, 4, 0.35),
                (6, 40, 64, 3, 0.9), (7, 33, 129, 3, 0.1)]


# ----------------------------------------------------------------------------- known answers
ROW_DISP = np.array([[3, 3, 9, 9, 9, -2, -2]], np.float32)


def test_occlusion_takes_the_largest_candidate():
    outl = np.array([[0, 0, 2, 2, 2, 0, 0]], np.uint8)
    out = interp_ref(ROW_DISP, outl, grey([[0] * 7]))
    assert out.tolist() == [[3, 3, 3, 3, 3, -2, -2]]


@pytest.mark.parametrize("colours", [(10, (190, 200, 215), 200), (90, (100, 100, 100), 110)], ids=["closer_right", "tie"])
def test_mismatch_takes_the_closest_colour_ties_to_the_earlier_direction(colours):
    left, mid, right = colours
    outl = np.array([[0, 0, 1, 1, 7, 0, 0]], np.uint8)
    img = grey([[left, left, mid[0], mid[1], mid[2], right, right]])
    out = interp_ref(ROW_DISP, outl, img)
    assert out.tolist() == [[3, 3, -2, -2, -2, -2, -2]]  # (1, 0) comes before (-1, 0)
    assert np.array_equal(interp_ref_fast(ROW_DISP, outl, img), out)


def test_all_outlier_map_is_unchanged():
    disp, _, img = random_case(11, 6, 9)
    outl = np.full(disp.shape, 2, np.uint8)
    outl[::2] = 1
    assert np.array_equal(interp_ref(disp, outl, img), disp, equal_nan=True)
    assert np.array_equal(interp_ref_fast(disp, outl, img), disp, equal_nan=True)


def test_knights_move_reaches_what_the_others_miss():
    """3 x 5, the only reliable pixel at (x = 4, y = 2): (0, 0) finds it through (2, 1), (1, 0) finds nothing"""
    disp = np.arange(15, dtype=np.float32).reshape(3, 5)
    outl = np.ones((3, 5), np.uint8)
    outl[2, 4] = 0
    outl[0, 1] = 2
    out = interp_ref(disp, outl, grey(np.zeros((3, 5))))
    assert out[0, 0] == disp[2, 4] and out[0, 1] == disp[0, 1]
    assert np.array_equal(interp_ref_fast(disp, outl, grey(np.zeros((3, 5)))), out)


def test_nan_follows_the_fold_order():
    """occlusion: NaN iff the first direction that has a candidate carries NaN, otherwise the largest non-NaN candidate"""
    nan = np.float32(np.nan)
    outl = np.array([[0, 2, 0]], np.uint8)
    img = grey([[0, 0, 0]])
    first_nan = interp_ref(np.array([[5, 1, nan]], np.float32), outl, img)  # (1, 0) first: NaN stays
    assert np.isnan(first_nan[0, 1])
    later_nan = interp_ref(np.array([[nan, 1, 5]], np.float32), outl, img)  # (1, 0) -> 5; NaN > 5 is false
    assert later_nan[0, 1] == 5
    for d in ([[5, 1, nan]], [[nan, 1, 5]]):
        d = np.array(d, np.float32)
        assert np.array_equal(interp_ref_fast(d, outl, img), interp_ref(d, outl, img), equal_nan=True)


@pytest.mark.parametrize("case", RANDOM_CASES, ids=["%dx%dx%d" % c[1:4] for c in RANDOM_CASES])
def test_fast_form_is_the_scalar_form(case):
    disp, outl, img = random_case(*case)
    want = interp_ref(disp, outl, img)
    got = interp_ref_fast(disp, outl, img)
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(got[outl == 0], disp[outl == 0], equal_nan=True)  # reliable pixels are never written
    assert not np.array_equal(want, disp, equal_nan=True)
    if min(disp.shape) > 1:
        assert set(np.unique(outl)) >= {0, 1, 2, 7}


# ----------------------------------------------------------------------------- the frame chain
def test_composed_chain_is_the_oracle_frame(orc):
    """interp_frame without the step is orc_adcensus_stm, with and without HSLO: the composition the GPU tests use is the frame's"""
    from stm_amd import synth
    H, W, D, zd = 40, 64, 16, 8
    p = _P(D, zd, usd=17, lsd=8)
    sbs, _ = synth.sbs_frame(H, W, D, zd)
    for hslo in (False, True):
        want = orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                                p.thresh_s, p.thresh_h, hslo=hslo)
        dl, dr, mux, _ = interp_frame(orc, sbs, p, 3, False, hslo=hslo)
        assert np.array_equal(dl, want["disp_l"]) and np.array_equal(dr, want["disp_r"]), hslo
        assert np.array_equal(mux, want["interlaced"]), hslo


def test_interpolated_maps_stay_whole_numbers_in_range(orc):
    """the step copies values of the map: what the integer-map bilateral filter is promised still holds after it"""
    from stm_amd import synth
    H, W, D, zd = 48, 100, 16, 8
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + 5)
    _, _, _, info = interp_frame(orc, sbs, _P(D, zd, usd=17, lsd=8), 2, True)
    for side in "lr":
        m = info["interp_" + side]
        assert np.array_equal(m, np.floor(m)) and m.min() >= -zd and m.max() <= D - 1 - zd
        rel = info["outl_" + side] == 0
        assert np.array_equal(m[rel], info["voted_" + side][rel])


# ----------------------------------------------------------------------------- quality against the true offsets
QUALITY = [("96x160_d16", 96, 160, 16, 8, 0, 17, 8), ("135x240_d32", 135, 240, 32, 16, 1, 34, 17)]


@pytest.mark.parametrize("case", QUALITY, ids=[c[0] for c in QUALITY])
def test_interpolation_brings_the_remaining_outliers_closer_to_the_truth(orc, case):
    """Left view, the pixels still marked after IRV x5, mean |disp - true offset| before -> after the step (share off by more
    than one pixel): 96 x 160, D = 16: 5.454 -> 3.165 (0.809 -> 0.469); 135 x 240, D = 32: 5.598 -> 3.332 (0.831 -> 0.451).
    The bound 0.75 leaves room for nothing but a bug (the definition itself gives 0.58 and 0.60)."""
    from stm_amd import synth
    name, H, W, D, zd, dseed, usd, lsd = case
    sbs, off = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + dseed)
    _, _, _, info = interp_frame(orc, sbs, _P(D, zd, usd=usd, lsd=lsd), 2, True)
    m = info["outl_l"] != 0
    assert m.sum() > 100, m.sum()
    before = float(np.mean(np.abs(info["voted_l"][m] - off[m])))
    after = float(np.mean(np.abs(info["interp_l"][m] - off[m])))
    far_b = float(np.mean(np.abs(info["voted_l"][m] - off[m]) > 1))
    far_a = float(np.mean(np.abs(info["interp_l"][m] - off[m]) > 1))
    print("%s: %d outliers, mean abs error %.3f -> %.3f, off by > 1 px %.3f -> %.3f" % (name, m.sum(), before, after, far_b, far_a))
    assert after < 0.75 * before, (before, after)
