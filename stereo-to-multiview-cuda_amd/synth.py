"""Seeded synthetic stereo pairs: value-noise left image, piecewise-constant
integer disparity field (background plane + rectangles), right image by forward mapping with z-order.

Convention: hypothesis index d means horizontal offset o = d - zero_disp and the left
cost pairs L(x) with R(x + o), so a left pixel with offset `off` appears in the right image at x + off.
"""
import numpy as np

SEED = 0x5EED0001


def _value_noise(rng, H, W, cell):
    gh, gw = H // cell + 2, W // cell + 2
    g = rng.random_sample((gh, gw)).astype(np.float32)
    ys = np.arange(H, dtype=np.float32) / cell
    xs = np.arange(W, dtype=np.float32) / cell
    y0 = np.floor(ys).astype(np.int64)
    x0 = np.floor(xs).astype(np.int64)
    fy = (ys - y0)[:, None]
    fx = (xs - x0)[None, :]
    fy = fy * fy * (3 - 2 * fy)
    fx = fx * fx * (3 - 2 * fx)
    a = g[y0][:, x0]
    b = g[y0][:, x0 + 1]
    c = g[y0 + 1][:, x0]
    d = g[y0 + 1][:, x0 + 1]
    return (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy


def left_image(H, W, seed=SEED):
    rng = np.random.RandomState(seed & 0x7FFFFFFF)
    base = 0.6 * _value_noise(rng, H, W, 64) + 0.3 * _value_noise(rng, H, W, 16) + 0.1 * _value_noise(rng, H, W, 4)
    img = np.empty((H, W, 3), np.float32)
    for c in range(3):
        own = 0.6 * _value_noise(rng, H, W, 64) + 0.3 * _value_noise(rng, H, W, 16) + 0.1 * _value_noise(rng, H, W, 4)
        img[:, :, c] = 0.7 * base + 0.3 * own
    lo, hi = img.min(), img.max()
    return np.clip((img - lo) / (hi - lo) * 255.0, 0, 255).astype(np.uint8)


def disparity_field(H, W, num_disp, zero_disp, seed=SEED, n_rect=12):
    rng = np.random.RandomState((seed ^ 0x9E3779B9) & 0x7FFFFFFF)
    lo, hi = -(zero_disp - 1) + 2, (num_disp - zero_disp - 1) - 2
    if lo > hi:
        lo = hi = 0
    off = np.full((H, W), max(min(-4, hi), lo), np.int32)
    for _ in range(n_rect):
        rh = int(H * rng.uniform(0.05, 0.25))
        rw = int(W * rng.uniform(0.05, 0.25))
        y0 = rng.randint(0, max(H - rh, 1))
        x0 = rng.randint(0, max(W - rw, 1))
        off[y0:y0 + rh, x0:x0 + rw] = rng.randint(lo, hi + 1)
    return off


def right_image(left, off):
    H, W, _ = left.shape
    right = np.zeros_like(left)
    filled = np.zeros((H, W), bool)
    xs = np.arange(W)[None, :].repeat(H, 0)
    for o in sorted(np.unique(off).tolist(), reverse=True):  # far (large o) first, near (very negative o) last
        m = off == o
        tx = xs + o
        ok = m & (tx >= 0) & (tx < W)
        yy, xx = np.nonzero(ok)
        right[yy, xx + o] = left[yy, xx]
        filled[yy, xx + o] = True
    # holes take the value of their left neighbour (first column: the left image's pixel)
    for x in range(W):
        h = ~filled[:, x]
        if not h.any():
            continue
        right[h, x] = left[h, x] if x == 0 else right[h, x - 1]
    return right


def stereo_pair(H, W, num_disp, zero_disp, seed=SEED):
    """Returns (left, right, offset_field): BGR u8 [H][W][3] x2 and the integer ground-truth offsets."""
    L = left_image(H, W, seed)
    off = disparity_field(H, W, num_disp, zero_disp, seed)
    R = right_image(L, off)
    return L, R, off


def sbs_frame(H, W, num_disp, zero_disp, seed=SEED):
    """Side-by-side frame [H][2W][3] as adcensus_stm expects (left half = left view, d_demux_common.cu:16-31)."""
    L, R, off = stereo_pair(H, W, num_disp, zero_disp, seed)
    return np.ascontiguousarray(np.concatenate([L, R], axis=1)), off


def tiled_pair(left, right, H, W):
    """A real-content stereo pair of any size from a small one (the reference's 640x384 img/bud_2 + bud_3): repeated
    horizontally (keeps the sign of every disparity), mirrored vertically on every other repeat (a vertical flip leaves
    a rectified pair rectified), cropped to H x W.  The seams are ordinary depth/colour edges; what matters is that arm
    lengths, outlier density and disparity statistics are those of real content (14.5 % L/R outliers on this pair against
    2 % on the value-noise frame)."""
    h, w, _ = left.shape
    ny, nx = (H + h - 1) // h, (W + w - 1) // w

    def tile(img):
        rows = [np.concatenate([img if (j % 2 == 0) else img[::-1] for _ in range(nx)], axis=1) for j in range(ny)]
        return np.ascontiguousarray(np.concatenate(rows, axis=0)[:H, :W])
    return tile(left), tile(right)


def tiled_sbs_frame(left, right, H, W):
    L, R = tiled_pair(left, right, H, W)
    return np.ascontiguousarray(np.concatenate([L, R], axis=1))


def pack_frame(left, right, packing=0, swap=0, gap=0, extra_cols=0, fill=0):
    """A packed BGR frame uint8 [rows_f][Wsbs][3] (include/stm_hip.h, stm_demux_packed) from a full-resolution pair uint8 [H][W][3]:
    packing 0 / 2 = the eyes side by side / one above the other, 1 / 3 = each eye first squeezed to half the columns / rows by
    averaging pairs ((a + b + 1) >> 1); swap: the right eye first; `gap` pixels of `fill` between the eyes along the packing axis and
    extra_cols columns of it past the row the rule asks for.  It only manufactures inputs, as a 3D encoder would: the expansion is
    the library's."""
    def squeeze(img, axis):
        a = np.moveaxis(img.astype(np.int32), axis, 0)
        return np.moveaxis(((a[0::2] + a[1::2] + 1) >> 1).astype(np.uint8), 0, axis)
    eyes = [left, right]
    if packing & 1:
        assert left.shape[1 if packing == 1 else 0] % 2 == 0
        eyes = [squeeze(e, 1 if packing == 1 else 0) for e in eyes]
    if swap:
        eyes = eyes[::-1]
    Hp, Wp, _ = eyes[0].shape
    rows, cols = (Hp, 2 * Wp + gap) if packing < 2 else (2 * Hp + gap, Wp)
    frame = np.full((rows, cols + extra_cols, 3), fill, np.uint8)
    frame[:Hp, :Wp] = eyes[0]
    if packing < 2:
        frame[:, Wp + gap:2 * Wp + gap] = eyes[1]
    else:
        frame[Hp + gap:, :Wp] = eyes[1]
    return frame


# (Kr, Kb), limited range?  -- the four conversion matrices of stm_demux_nv12, in its numbering
NV12_MATRICES = ((0.299, 0.114, True), (0.2126, 0.0722, True), (0.299, 0.114, False), (0.2126, 0.0722, False))


def bgr_to_nv12(frame, matrix=0):
    """A BGR frame uint8 [H][W][3] (H, W even) as NV12: (y uint8 [H][W], uv uint8 [H / 2][W], U and V interleaved), chroma
    the mean of each 2 x 2 block, in floating point and rounded.  It only manufactures inputs for the NV12 calls: the exact
    integer conversion is the library's, in the other direction."""
    kr, kb, limited = NV12_MATRICES[matrix]
    kg = 1.0 - kr - kb
    H, W, _ = frame.shape
    assert H % 2 == 0 and W % 2 == 0
    b, g, r = (frame[:, :, c].astype(np.float64) for c in range(3))
    yf = kr * r + kg * g + kb * b
    u = (b - yf) / (2.0 * (1.0 - kb))
    v = (r - yf) / (2.0 * (1.0 - kr))
    ys, cs, yo = (219.0 / 255.0, 224.0 / 255.0, 16.0) if limited else (1.0, 1.0, 0.0)
    y = np.clip(np.rint(yf * ys + yo), 0, 255).astype(np.uint8)
    uv = np.empty((H // 2, W), np.uint8)
    for k, c in enumerate((u, v)):
        m = c.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))
        uv[:, k::2] = np.clip(np.rint(m * cs + 128.0), 0, 255).astype(np.uint8)
    return y, uv
