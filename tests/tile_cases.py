"""Inputs for the tests of the stencil filters' tile forms (tests/test_tile_shortcuts_ref.py, tests/test_gpu_tile_shortcuts.py), and
a numpy restatement of the geometry the two kernels decide on.

stm_k_gaussian_max_r<R> and stm_k_bilateral_r<7, INTMAP> (csrc/stm_kernels_refine.hip) inspect a block's tile while loading it and
then pick a form for the whole block: the gaussian kernel stores c where tile and halo hold one value c in {0, 1}; the bilateral
kernel takes its integer form where every value is a whole number below 2^19 in size and max - min < ncolor, and stores one number
where in addition min == max.  A wrong decision gives plausible numbers, and only in a map that is uniform up to the edge of what
the block needs.  The builders here make such maps: a uniform map with ONE different pixel (or line) on, and just beyond, every
edge of one block's needed neighbourhood.

Geometry: a block covers BW x BH = 64 x 16 output pixels; the block at (x0, y0) NEEDS columns x0 - R .. x0 + 63 + R and rows
y0 - R .. y0 + 15 + R, clamped into the image, and SCANS tile_width(R) columns from x0 - R on (6 more to the right than needed at
R = 7, 4 more at R = 10): a different value in those padding columns may make the kernel run its stencil, never change a result.
The standard map is 48 x 192 = 3 x 3 blocks; its middle block has a full, unclamped halo at R = 7 and R = 10.

Every case is (name, map, inside): inside = True where the different value lies in the middle block's needed neighbourhood (the
expected output of that block must then differ from the unperturbed map's, or a shortcut taken by mistake would not show), False
where it lies outside (the block's output must be the unperturbed one: the shortcut is legitimate), None where the case makes no
such statement.  test_tile_shortcuts_ref.py asserts exactly that on the oracle.
"""
import functools

import numpy as np

BW, BH = 64, 16
STD_H, STD_W = 48, 192
X0, Y0 = 64, 16  # the middle block of the standard map
EDGE_SHAPES = [(1, 1), (16, 64), (15, 63), (17, 65), (33, 70), (48, 130)]
GAUSS_FAST = [(10, 15.0), (7, 10.0)]  # the (radius, sigma) pairs that take stm_k_gaussian_max_r
GAUSS_GENERIC = (3, 2.0)              # ... and one that takes the generic kernel, on the same maps
BIL = (7, 5.0, 10.0)                  # radius, sigma_color, sigma_spatial of the frame's bilateral filter
BIL_D = 16
LIMIT = 1 << 19                       # the integer form takes |value| < 2^19


# ----------------------------------------------------------------------------- geometry
def tile_width(R):
    return (BW + 2 * R + 3) // 4 * 4 + 4


def blocks(H, W):
    return [(y0, x0) for y0 in range(0, H, BH) for x0 in range(0, W, BW)]


def needed(H, W, R, y0, x0):
    """(rows, cols) index arrays of the pixels the block at (y0, x0) needs, clamped (with repeats) into the image"""
    return np.clip(np.arange(y0 - R, y0 + BH + R), 0, H - 1), np.clip(np.arange(x0 - R, x0 + BW + R), 0, W - 1)


def scanned(H, W, R, y0, x0):
    """(rows, cols) of the pixels the block inspects: the needed ones and the padding columns"""
    return np.clip(np.arange(y0 - R, y0 + BH + R), 0, H - 1), np.clip(np.arange(x0 - R, x0 - R + tile_width(R)), 0, W - 1)


def in_needed(R, y, x, y0=Y0, x0=X0):
    return y0 - R <= y <= y0 + BH - 1 + R and x0 - R <= x <= x0 + BW - 1 + R


def block_of(a, y0=Y0, x0=X0):
    return a[y0:y0 + BH, x0:x0 + BW]


def one_value_blocks(m, R):
    """[(y0, x0, value)] of the blocks whose scanned region holds one value"""
    H, W = m.shape
    out = []
    for y0, x0 in blocks(H, W):
        t = m[np.ix_(*scanned(H, W, R, y0, x0))]
        if (t == t.flat[0]).all():
            out.append((y0, x0, float(t.flat[0])))
    return out


# ----------------------------------------------------------------------------- one different pixel
def band_positions(R):
    """(y, x) of the sweep around the middle block of the standard map: a band across each edge of its needed neighbourhood at two
    rows / columns inside the block, the four halo corners with their diagonal neighbours outside, one pixel inside the block"""
    pos = []
    for y in (Y0 + 5, Y0 + 12):
        pos += [(y, x) for x in range(X0 - R - 2, X0 - R + 2)]
        pos += [(y, x) for x in range(X0 + BW - 1 + R - 1, X0 + BW - 1 + R + 9)]
    for x in (X0 + 9, X0 + 50):
        pos += [(y, x) for y in range(Y0 - R - 2, Y0 - R + 2)]
        pos += [(y, x) for y in range(Y0 + BH - 1 + R - 1, Y0 + BH - 1 + R + 3)]
    for cy, sy in ((Y0 - R, -1), (Y0 + BH - 1 + R, 1)):
        for cx, sx in ((X0 - R, -1), (X0 + BW - 1 + R, 1)):
            pos += [(cy, cx), (cy + sy, cx + sx)]
    pos.append((Y0 + 7, X0 + 30))
    assert all(0 <= y < STD_H and 0 <= x < STD_W for y, x in pos) and len(set(pos)) == len(pos)
    return pos


def uniform(H, W, v):
    return np.full((H, W), v, np.float32)


def pixel_sweep(R, base, pixel):
    """the standard map of `base` with `pixel` at one position of the sweep per case"""
    for y, x in band_positions(R):
        m = uniform(STD_H, STD_W, base)
        m[y, x] = pixel
        yield "base%g_px%g_y%d_x%d" % (base, pixel, y, x), m, in_needed(R, y, x)


def edge_shape_cases(base, pixel):
    """every edge shape: the uniform map, and `pixel` at each image corner and at the first pixel of the last, partial block"""
    for H, W in EDGE_SHAPES:
        yield "%dx%d_base%g" % (H, W, base), uniform(H, W, base), None
        spots = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), ((H - 1) // BH * BH, (W - 1) // BW * BW)}
        for y, x in sorted(spots):
            m = uniform(H, W, base)
            m[y, x] = pixel
            yield "%dx%d_base%g_px%g_y%d_x%d" % (H, W, base, pixel, y, x), m, None


# ----------------------------------------------------------------------------- A: gaussian, non-inverted
GAUSS_UNIFORM = [0.0, 1.0, 0.5, 2.0, -1.0]  # 0 and 1 take the shortcut, the others must not
# the filter is grow-only, out = max(in, blur): the pixel must RAISE the blur above the base to show in its neighbours
GAUSS_PERTURB = [(0.0, 1.0), (1.0, 2.0)]


def gauss_thirds():
    """left third 0, middle third 1, right third random 0 / 1.  On three block columns every block's scanned region crosses a
    step, so all nine blocks run the stencil next to a step of the map: gauss_mixed is the map on which the shortcuts fire"""
    m = np.zeros((STD_H, STD_W), np.float32)
    m[:, BW:2 * BW] = 1.0
    m[:, 2 * BW:] = (np.random.RandomState(3).random_sample((STD_H, BW)) > 0.5).astype(np.float32)
    return m


def gauss_mixed(R):
    """random 0 / 1, but 0 over exactly the scanned region of the top-left block and 1 over exactly that of the bottom-right one:
    one block stores 0, one stores 1, the seven others run the stencil, and the neighbours of the two have a halo that leaves
    the uniform region one pixel beyond what the shortcut blocks inspect"""
    m = (np.random.RandomState(3).random_sample((STD_H, STD_W)) > 0.5).astype(np.float32)
    ys, xs = scanned(STD_H, STD_W, R, 0, 0)
    m[np.ix_(ys, xs)] = 0.0
    ys, xs = scanned(STD_H, STD_W, R, STD_H - BH, STD_W - BW)
    m[np.ix_(ys, xs)] = 1.0
    return m


def gauss_cases(R):
    for b in GAUSS_UNIFORM:
        yield "uniform%g" % b, uniform(STD_H, STD_W, b), None
    for base, pixel in GAUSS_PERTURB:
        yield from pixel_sweep(R, base, pixel)
    yield "thirds", gauss_thirds(), None
    yield "mixed", gauss_mixed(R), None
    for base, pixel in GAUSS_PERTURB:
        yield from edge_shape_cases(base, pixel)


# ----------------------------------------------------------------------------- B: gaussian, inverted (dibr_dbm's blend mask)
DBM_SHIFT = 0.5
# (mask_r base, line value): after the fused 1 - x the base is 0 / 1 and the line 1 / 2, which raises the blur
DBM_PERTURB = [(1.0, 0.0), (0.0, -1.0)]


def dbm_inputs(H=STD_H, W=STD_W):
    """img_l, img_r, disp_l, disp_r, mask_l: the view is then a blend of 0 and 255 by the blurred, inverted mask_r alone
    (mask_l = 1: with mask_l = 0 the blend does not reach the output)"""
    z = np.zeros((H, W), np.float32)
    return np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8), z, z.copy(), np.ones((H, W), np.float32)


def dbm_lines(R):
    """(name, rows, cols, inside): a line of 64 pixels (a column: the map's 48 rows) on the outermost needed halo row / column of
    the middle block, and one row / column beyond it"""
    out = []
    xs, ys = slice(X0, X0 + BW), slice(0, STD_H)
    for name, y in (("top", Y0 - R), ("bottom", Y0 + BH - 1 + R)):
        beyond = y + (-1 if name == "top" else 1)
        out += [(name, slice(y, y + 1), xs, True), (name + "_beyond", slice(beyond, beyond + 1), xs, False)]
    for name, x in (("left", X0 - R), ("right", X0 + BW - 1 + R)):
        beyond = x + (-1 if name == "left" else 1)
        out += [(name, ys, slice(x, x + 1), True), (name + "_beyond", ys, slice(beyond, beyond + 1), False)]
    return out


def dbm_cases(R):
    """(name, mask_r, inside)"""
    for base, line in DBM_PERTURB:
        yield "mask%g" % base, uniform(STD_H, STD_W, base), None
        for name, rows, cols, inside in dbm_lines(R):
            m = uniform(STD_H, STD_W, base)
            m[rows, cols] = line
            yield "mask%g_line%g_%s" % (base, line, name), m, inside


# ----------------------------------------------------------------------------- C: bilateral forms
BIL_UNIFORM = [0.0, 1.0, -1.0, BIL_D - 1.0, -(LIMIT - 1.0), LIMIT - 1.0,  # one-value form
               float(-LIMIT),                                              # the scan's unsigned compare takes -2^19 too
               float(LIMIT), -LIMIT - 1.0,                                 # flagged: general form
               0.5]                                                        # a fraction: general form
BIL_SWEEP_BASES = [5.0, -3.0]


def bil_range_cases(D=BIL_D):
    """Whole numbers whose range is exactly D - 1 (integer form, the colour LUT's last entry) and exactly D (general form, the
    clamped index): as one pixel at a halo corner of the middle block -- the block's corner pixel then sees the full difference
    -- as min and max at opposite halo corners, as a step through the block, and with the larger value in the scanned padding
    columns only (not needed: the form may change, the block's result may not)"""
    R = BIL[0]
    tl, br = (Y0 - R, X0 - R), (Y0 + BH - 1 + R, X0 + BW - 1 + R)
    for a in (0.0, -9.0, LIMIT - 1.0 - D):
        for span in (D - 1, D):
            for name, (y, x) in (("tl", tl), ("br", br)):
                m = uniform(STD_H, STD_W, a)
                m[y, x] = a + span
                yield "a%g_span%d_%s" % (a, span, name), m, True
            m = uniform(STD_H, STD_W, a + 7)
            m[tl], m[br] = a, a + span
            yield "a%g_span%d_opposite" % (a, span), m, True
            m = uniform(STD_H, STD_W, a)
            m[:, X0 + 30:] = a + span
            yield "a%g_span%d_step" % (a, span), m, True
            m = uniform(STD_H, STD_W, a)
            m[Y0 + 5, X0 + BW - 1 + R + 3] = a + span
            yield "a%g_span%d_padding" % (a, span), m, False


def bil_cases():
    R = BIL[0]
    for c in BIL_UNIFORM:
        yield "uniform%g" % c, uniform(STD_H, STD_W, c), None
    for c in BIL_SWEEP_BASES:
        yield from pixel_sweep(R, c, c + 1.0)
        yield from pixel_sweep(R, c, c + 0.5)  # the fraction must send the block to the general form
    yield from bil_range_cases()
    for c in BIL_SWEEP_BASES:
        yield from edge_shape_cases(c, c + 1.0)


# ----------------------------------------------------------------------------- D: every entry of the one-value table
# (H, W, D, zd): a pair with the constant shift s = -v gives maps that hold v over whole blocks, for every v in [-zd, D - zd)
TABLE_CONFIGS = [(48, 192, 64, 32), (48, 192, 64, 10), (40, 150, 20, 0), (48, 192, 130, 64)]
TABLE_USD, TABLE_LSD = 17, 8


class Params:
    """device_api.FrameParams' defaults without importing torch"""

    def __init__(self, num_disp, zero_disp, usd=TABLE_USD, lsd=TABLE_LSD):
        self.num_disp, self.zero_disp, self.num_views, self.angle = num_disp, zero_disp, 8, 18.43
        self.ad_coeff, self.census_coeff, self.ucd, self.lcd, self.usd, self.lsd = 10.0, 30.0, 6.0, 20.0, usd, lsd
        self.thresh_s, self.thresh_h, self.out_rows, self.out_cols = 20, 0.4, None, None


def table_values(cfg):
    _, _, D, zd = cfg
    return list(range(-zd, D - zd))


def table_stage3_values(cfg):
    v = table_values(cfg)
    return sorted({v[0], 0, v[-1]})


def table_pair(cfg, v):
    """side-by-side frame whose right view is the left one moved by the constant shift s = -v"""
    H, W, D, _ = cfg
    base = np.random.RandomState(1).randint(0, 256, size=(H, W + 2 * D, 3)).astype(np.uint8)
    s = -v
    return np.ascontiguousarray(np.concatenate([base[:, D:D + W], base[:, D + s:D + s + W]], axis=1))


@functools.lru_cache(maxsize=None)
def table_frames(orc, cfg):
    """{v: (sbs, disp_l, disp_r, voted_l, voted_r)}: the oracle's frame at stages = 2 for every v, and the maps that enter its
    bilateral filter.  Computed once per configuration; nobody writes to the arrays."""
    from test_interp_ref import interp_frame
    _, _, D, zd = cfg
    out = {}
    for v in table_values(cfg):
        sbs = table_pair(cfg, v)
        dl, dr, _, info = interp_frame(orc, sbs, Params(D, zd), 2, False)
        out[v] = (sbs, dl, dr, info["voted_l"], info["voted_r"])
        for a in out[v]:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def table_frame3(orc, cfg, v):
    """(disp_l, disp_r, interlaced) of the oracle's whole frame (stages = 3)"""
    from test_interp_ref import interp_frame
    _, _, D, zd = cfg
    return interp_frame(orc, table_pair(cfg, v), Params(D, zd), 3, False)[:3]
