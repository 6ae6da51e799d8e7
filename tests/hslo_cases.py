"""Inputs of the scanline optimisation's path-cost tests (tests/test_gpu_hslo_sums.py on the GPU, tests/test_oracle_second_opinion.py
on the CPU): images, cost volumes, the parameter sets, and the count of penalty classes that says whether an input exercises them.
No test in here; numpy only.

Images.  A grey image hides the difference between the own image's integer mean and the other image's float mean, and a uniform
random image puts nearly every colour step above T = 15.  palette_image draws each pixel's channel sum B + G + R from PALETTE and
splits it unevenly over the channels: the means are then
    own (integer)  60  60      65  65      75  75      90
    other (float)  60  60.33   65  65.67   75  75.33   90
so steps land below T = 15 (0, 1/3, 5, 10, ...), on it (60 -> 75, 75 -> 90) and above it (25, 30, and 60.33 -> 75.33, which float32
rounds to 15.000004), differently for the two means."""
import numpy as np

PALETTE = (180, 181, 195, 197, 225, 226, 270)

# (T, H1, H2): the frame's constants; P1 > P2; H / 4 and H / 10 not exact in float32; no step below T; every step below T; no
# penalty at all; and a T that only unit_step_image's steps of exactly 1 in the channel sum can straddle (THIRD)
THIRD = float(np.float32(1.0) / np.float32(3.0))
PARAM_SETS = {
    "frame_15_1_3": (15.0, 1.0, 3.0),
    "p1_above_p2": (15.0, 3.0, 1.0),
    "inexact_quarters": (7.5, 0.3, 7.1),
    "t_zero": (0.0, 1.0, 3.0),
    "t_huge": (1e9, 1.0, 3.0),
    "no_penalty": (15.0, 0.0, 0.0),
    "t_one_third": (THIRD, 1.0, 3.0),
}


# The kernel forms (tests/test_gpu_hslo_sums.py) and stm_set_agg_variant's word of each, and the walk-geometry cases (form, H, W):
# W -> G = ceil(W / 4): 1, 3, 4 -> 1;  5 -> 2;  9 -> 3;  13 -> 4;  17 -> 5;  29 -> 8;  33, 36 -> 9;  38 -> 10: G = 1, and G below / equal
# to / one above the prefetch depth of each form (h2: 4, h1: 8, dpl2: 4, dpl4: 2), odd and even G for the two-ended handover in the
# middle of the row, and (W % 4 != 0) a last group partly outside the image, the first group the right-to-left walk enters.  9 and
# 29 are added to the widths the forms were asked at, for G = 3 (one above dpl4's depth) and G = 8 (h1's depth itself).  H around the
# vertical kernels' prefetch depths 8, 4, 2.  Each W once per form, the heights dealt round.
FORMS = {"h2": 0, "h1": 400, "dpl2": 0, "dpl4": 0}
GEO_W = [1, 3, 4, 5, 9, 13, 17, 29, 33, 36, 38]
GEO_H = [1, 2, 3, 8, 9, 17]
GEO_D = {"h2": (7, 3), "h1": (7, 3), "dpl2": (70, 30), "dpl4": (130, 64)}  # (D, zero_disp)
GEO = [(form, GEO_H[(i + 2 * k) % len(GEO_H)], W) for k, form in enumerate(sorted(FORMS)) for i, W in enumerate(GEO_W)]


def geo_can_cover(H, W):
    """the walk-geometry shapes large enough to hold every class pair eight times per direction at D = 7 (over 1400 (step,
    hypothesis) slots per direction; the rarest pair, a step of exactly 15 in both images, has a probability near 0.02)"""
    return H >= 8 and W >= 29


def _split(s, rng, elem_sz):
    """channel sums [H][W] -> uint8 [H][W][elem_sz], B + G + R = s, unevenly: about a half, a third and the rest"""
    k = rng.randint(0, 6, size=s.shape)
    b = s // 2 - k
    g = s // 3 + k
    r = s - b - g
    img = np.zeros(s.shape + (elem_sz,), np.uint8)
    assert b.min() >= 0 and g.min() >= 0 and r.min() >= 0 and max(b.max(), g.max(), r.max()) <= 255
    img[..., 0], img[..., 1], img[..., 2] = b, g, r
    if elem_sz > 3:
        img[..., 3:] = rng.randint(0, 256, size=s.shape + (elem_sz - 3,))  # a fourth byte no mean may look at
    return img


def palette_image(H, W, seed, elem_sz=3):
    rng = np.random.RandomState(seed)
    s = np.asarray(PALETTE)[rng.randint(0, len(PALETTE), size=(H, W))]
    return _split(s, rng, elem_sz)


def unit_step_image(H, W, seed, elem_sz=3):
    """channel sums a[x] + b[y] of two random +-1 walks: every horizontal and every vertical neighbour differs by exactly 1, so the
    integer mean steps by 0 or 1 and the float mean by float32(s / 3) - float32((s - 1) / 3), just below or just above float32(1/3)"""
    rng = np.random.RandomState(seed)
    a = np.cumsum(rng.choice([-1, 1], size=W))
    b = np.cumsum(rng.choice([-1, 1], size=H))
    s = 300 + a[None, :] + b[:, None]
    return _split(s, rng, elem_sz)


def means(img_own, img_other):
    """(own, other) float32 [H][W] as the definition takes them: integer mean as u8; float32 of (float32 sum / 3.0 in double)"""
    so = img_own[..., :3].astype(np.int64).sum(axis=2)
    st = img_other[..., :3].astype(np.int64).sum(axis=2)
    return (so // 3).astype(np.float32), (st.astype(np.float32).astype(np.float64) / 3.0).astype(np.float32)


def _cls(a, b, T):
    s = np.abs(a - b)  # float32
    T = np.float32(T)
    return np.where(s < T, 0, np.where(s > T, 1, 2))


def class_counts(img_own, img_other, D, zd, osign, T):
    """int [4][3][3]: per direction (left->right, right->left, top->bottom, bottom->top) how many (step, hypothesis) take the class
    pair (class D1, class D2); class 0 = step < T, 1 = step > T, 2 = neither"""
    mo, mt = means(img_own, img_other)
    H, W = mo.shape
    xs = np.arange(W)
    out = np.zeros((4, 3, 3), np.int64)
    for k, (dx, dy) in enumerate([(1, 0), (-1, 0), (0, 1), (0, -1)]):
        ys = np.arange(H)
        x = xs[(xs - dx >= 0) & (xs - dx < W)]
        y = ys[(ys - dy >= 0) & (ys - dy < H)]
        if not len(x) or not len(y):
            continue
        c1 = _cls(mo[np.ix_(y, x)], mo[np.ix_(y - dy, x - dx)], T)
        for d in range(D):
            o = osign * (d - zd)
            qx, qpx = np.clip(x + o, 0, W - 1), np.clip(x - dx + o, 0, W - 1)
            c2 = _cls(mt[np.ix_(y, qx)], mt[np.ix_(y - dy, qpx)], T)
            np.add.at(out[k], (c1.ravel(), c2.ravel()), 1)
    return out


def assert_all_class_pairs(img_own, img_other, D, zd, osign, T=15.0, at_least=8):
    """a condition on the INPUT: all nine (class D1, class D2) pairs occur in each of the four directions, at_least times each"""
    n = class_counts(img_own, img_other, D, zd, osign, T)
    assert n.min() >= at_least, "an input that leaves a penalty class pair unexercised: counts per direction\n%s" % n


def covering_images(H, W, D, zd, seed, elem_sz=3, tries=200):
    """(own, other) palette images of different seeds, the first pair from `seed` on that meets assert_all_class_pairs for both views at
    T = 15: at the smallest shapes not every draw holds the rarest pair (a step of exactly 15 in both images) eight times in every
    direction.  Deterministic; the tests assert the condition again on what they are given."""
    for s in range(seed, seed + tries):
        own, other = palette_image(H, W, s, elem_sz), palette_image(H, W, s + 100003, elem_sz)
        if min(class_counts(own, other, D, zd, osign, 15.0).min() for osign in (1, -1)) >= 8:
            return own, other
    raise AssertionError("no covering palette pair at %d x %d, D = %d, zero_disp = %d" % (H, W, D, zd))


def cost_volume(kind, D, H, W, seed):
    """float32 [D][H][W], finite.  uniform: [0, 3).  quarters: the same in multiples of 0.25 -- exact ties in the minima and in WTA.
    constant: every map value is -zero_disp (at D > 64 the cross-lane tie path of WTA).  scaled: [0, 3e6), where (C + best) - m in the
    other order rounds differently.  planted: [1, 3) with each pixel's minimum 0 planted at one of d = 0, 63, 64, 127, 128, D - 1."""
    rng = np.random.RandomState(seed)
    c = (rng.random_sample((D, H, W)) * 3).astype(np.float32)
    if kind == "quarters":
        c = (np.floor(c * 4) / 4).astype(np.float32)
    elif kind == "constant":
        c[:] = np.float32(1.75)
    elif kind == "scaled":
        c = (c * np.float32(1e6)).astype(np.float32)
    elif kind == "planted":
        c = (1 + c * np.float32(2.0 / 3.0)).astype(np.float32)
        spots = np.asarray(sorted({d for d in (0, 63, 64, 127, 128, D - 1) if d < D}))
        pick = spots[rng.randint(0, len(spots), size=(H, W))]
        np.put_along_axis(c, pick[None], np.float32(0.0), axis=0)
    else:
        assert kind == "uniform", kind
    return c
