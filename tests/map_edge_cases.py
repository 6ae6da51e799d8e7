"""Disparity maps with huge and non-finite values for the stages that take a caller's map: dr_dcc, dr_irv, filter_bilateral_1,
filter_median, dibr_occl and dibr_dfm ("Map values a stage cannot place").  Plain numpy, no GPU: test_map_edges_ref.py
checks on the oracle that the cases see what they are for, test_gpu_map_edges.py runs them through the library.

A case is a pair of maps (or one map with outliers and arms, for region voting) built from a seeded base map with a few PLANTED
values.  Planted values: NaN, +-inf, +-FLT_MAX, +-3e9, +-2^31, +-2147483520 (the largest float below 2^31), +-(W - 1), +-W,
+-(W + 0.5), +-0.999, -0.0 and +-1e-40.  Places: columns 0, 1, W / 2, W - 2 and W - 1 of the first, a middle and the last row,
wherever they exist.  No two planted values of one map share a 15 x 15 window (the reach of the bilateral at radius 7 and of a
cross region with arms of at most USD = 7) unless the case says so: the places of a shape are dealt into groups of places that
lie at least WIN apart, a case takes one group, and as k runs over the values every place of the group meets every value.
"""
import numpy as np

SHAPES = [(1, 1), (1, 2), (3, 5), (9, 37), (33, 257), (5, 300)]
WIN = 15
USD, LSD = 7, 3                 # arm limits of the region-voting cases: a cross region stays inside one window
IRV_RANGES = [(8, 4), (70, 0)]  # (D, zd): max(D, 65) = 65 and 70 histogram bins
BIL_D, BIL_ZD = 8, 4            # the bilateral's colour table has BIL_D entries
FLT_MAX = float(np.finfo(np.float32).max)
BELOW_2_31 = 2147483520.0
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def planted_values(W):
    big = [np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX, 3e9, -3e9, 2147483648.0, -2147483648.0, BELOW_2_31, -BELOW_2_31]
    row = [W - 1, -(W - 1), W, -W, W + 0.5, -(W + 0.5), 0.999, -0.999, -0.0, 1e-40, -1e-40]
    return np.array(big + row, np.float32)


N_VALUES = len(planted_values(2))
# values that no histogram of region voting has a bin for, whatever (D, zd) of IRV_RANGES: f2i_sat(v) + zd is far outside [0, nb)
NO_BIN = np.array([3e9, -3e9, np.inf, -np.inf, FLT_MAX, -FLT_MAX, 2147483648.0, -2147483648.0], np.float32)


def places(H, W):
    rows = sorted({0, H // 2, H - 1})
    cols = sorted(c for c in {0, 1, W // 2, W - 2, W - 1} if 0 <= c < W)
    return [(y, x) for y in rows for x in cols]


def _far(p, q):
    return abs(p[0] - q[0]) >= WIN or abs(p[1] - q[1]) >= WIN


def place_groups(H, W):
    """the places dealt into groups whose members lie pairwise at least WIN apart in rows or in columns"""
    groups = []
    for p in places(H, W):
        for g in groups:
            if all(_far(p, q) for q in g):
                g.append(p)
                break
        else:
            groups.append([p])
    return groups


def base_map(H, W, seed, lo=-3, hi=4, fraction=True):
    rng = np.random.RandomState(seed)
    m = rng.randint(lo, hi, size=(H, W)).astype(np.float32)
    if fraction:
        m = m + (rng.random_sample((H, W)) * 0.9).astype(np.float32)
    return m.astype(np.float32)


def _freeze(*arrs):
    for a in arrs:
        a.setflags(write=False)


_PAIRS = {}


def pair_cases(H, W, whole=False):
    """[(name, disp_l, disp_r, planted)]: planted = [(map 0 / 1, y, x, value)].  Both maps carry planted values, the right map at
    the places of the next group and with other values.  whole: base maps of whole numbers in [-BIL_ZD, BIL_D - BIL_ZD)."""
    key = (H, W, whole)
    if key in _PAIRS:
        return _PAIRS[key]
    vals, groups = planted_values(W), place_groups(H, W)
    lo, hi = (-BIL_ZD, BIL_D - BIL_ZD) if whole else (-3, 4)
    bl = base_map(H, W, 1000 * H + W, lo, hi, not whole)
    br = base_map(H, W, 1000 * H + W + 1, lo, hi, not whole)
    cases = []
    for gi, g in enumerate(groups):
        gr = groups[(gi + 1) % len(groups)]
        for k in range(N_VALUES):
            dl, dr, planted = bl.copy(), br.copy(), []
            for j, (y, x) in enumerate(g):
                dl[y, x] = vals[(k + 5 * j) % N_VALUES]
                planted.append((0, y, x, dl[y, x]))
            for j, (y, x) in enumerate(gr):
                dr[y, x] = vals[(k + 11 + 7 * j) % N_VALUES]
                planted.append((1, y, x, dr[y, x]))
            _freeze(dl, dr)
            cases.append(("%dx%d_g%d_k%d" % (H, W, gi, k), dl, dr, planted))
    _PAIRS[key] = cases
    return cases


def images(H, W, elem_sz):
    """a seeded image pair with elem_sz bytes per pixel (dibr_dfm copies the first three)"""
    rng = np.random.RandomState(7 * H + W)
    il = rng.randint(1, 256, size=(H, W, elem_sz)).astype(np.uint8)   # no zero byte: a hole (0) is never mistaken for a pixel
    ir = rng.randint(1, 256, size=(H, W, elem_sz)).astype(np.uint8)
    _freeze(il, ir)
    return il, ir


# ---------------------------------------------------------------- region voting
_ARMS, _IRV = {}, {}


def arms(orc, H, W):
    """cross arms [4][H][W] of a seeded image (orc.ca_cross on conftest.rand_pair), arms of at most USD"""
    if (H, W) not in _ARMS:
        from conftest import rand_pair
        L, _ = rand_pair(H, W, 5 + H + W)
        cross, _ = orc.ca_cross(L, np.zeros((1, H, W), np.float32), 6.0, 20.0, USD, LSD)
        assert cross.max() <= USD
        _freeze(cross)
        _ARMS[(H, W)] = cross
    return _ARMS[(H, W)]


def _window(H, W, y, x):
    r = WIN // 2
    return slice(max(y - r, 0), min(y + r + 1, H)), slice(max(x - r, 0), min(x + r + 1, W))


def irv_cases(orc, H, W, D, zd):
    """[(name, kind, disp, outliers, cross, planted)] for dr_irv.  The base map holds whole numbers in [-zd, D - zd); about a third
    of the pixels inside the planted places' windows are outliers (classes 1 and 2), few elsewhere.  Kinds:
      vote   the planted values sit on reliable pixels, so they vote (or count towards the region's size only);
      own    the planted values sit on outliers: the `own` disparity an outlier keeps when nothing in its region has a bin;
      alone  as `own`, and this case SAYS SO: every reliable pixel of the planted outlier's window carries a value of NO_BIN, so
             that nothing votes, the winner is f2i_sat(own) and the accept ratio's numerator is f2i_sat(own) + zd.
    One case per value k; the places rotate with k through the shape's groups."""
    key = (H, W, D, zd)
    if key in _IRV:
        return _IRV[key]
    cross, vals, groups = arms(orc, H, W), planted_values(W), place_groups(H, W)
    base = base_map(H, W, 77 * H + W + D, -zd, D - zd, False)
    rng = np.random.RandomState(H + 31 * W + D)
    dense = np.zeros((H, W), bool)
    for (y, x) in places(H, W):
        dense[_window(H, W, y, x)] = True
    u = rng.random_sample((H, W))
    outl0 = np.where(u < np.where(dense, 0.35, 0.02), rng.randint(1, 3, size=(H, W)), 0).astype(np.uint8)
    cases = []
    for kind in ("vote", "own", "alone"):
        for k in range(N_VALUES):
            g = groups[k % len(groups)]
            disp, outl, planted = base.copy(), outl0.copy(), []
            for j, (y, x) in enumerate(g):
                if kind == "alone":
                    wy, wx = _window(H, W, y, x)
                    n = disp[wy, wx].size
                    disp[wy, wx] = NO_BIN[(np.arange(n) + k + j) % len(NO_BIN)].reshape(disp[wy, wx].shape)
                    if outl[wy, wx].all():            # the region needs a reliable pixel to have a size at all
                        ny, nx = (y, x + 1) if x + 1 < W else (y, max(x - 1, 0))
                        outl[ny, nx] = 0
                disp[y, x] = vals[(k + 5 * j) % N_VALUES]
                outl[y, x] = 0 if kind == "vote" else 1 + (k + j) % 2
                planted.append((0, y, x, disp[y, x]))
            _freeze(disp, outl)
            cases.append(("%dx%d_D%d_%s_k%d" % (H, W, D, kind, k), kind, disp, outl, cross, planted))
    _IRV[key] = cases
    return cases


# ---------------------------------------------------------------- the rules, restated
def f2i_sat(v):
    """float -> int of a map value: truncate toward zero, saturate at INT_MIN / INT_MAX, NaN -> 0.  int64 array: sums of two such
    values and an image coordinate cannot overflow."""
    v = np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        t = np.clip(np.trunc(np.where(np.isnan(v), 0.0, v)), float(INT_MIN), float(INT_MAX))
    return t.astype(np.int64)


def wrap32(a):
    """what a 32-bit register holds after the sum: the restatements' `wrap` variants put every sum through this"""
    return ((np.asarray(a, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def same(got, want):
    """equal, NaNs compared by position"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind == "f":
        return bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))
    return bool(np.array_equal(got, want))
