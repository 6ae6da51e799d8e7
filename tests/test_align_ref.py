"""The numpy statement of the vertical alignment (stm_set_align, stm_align_rows, stm_align_fit; include/stm_hip.h has the same
definition line by line) and its own checks on the CPU: apply, measure, fit, and the recovery of known fields from the two committed
pairs.  tests/test_gpu_align.py compares the kernels with these functions bit for bit."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

KB, KR = 8, 4  # column bands, row blocks
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- apply
def field_q(H, W, a, b, c):
    """q = the offset in sixteenths of a row, H x W int32: f32, one operation per line, rounded half up, clamped to +-16*64"""
    a, b, c = F32(a), F32(b), F32(c)
    u = np.arange(W, dtype=F32) - F32(0.5) * F32(W - 1)
    v = np.arange(H, dtype=F32) - F32(0.5) * F32(H - 1)
    t = (b * u)[None, :]
    s = a + t
    t = (c * v)[:, None]
    s = s + t
    m = s * F32(16)
    m = m + F32(0.5)
    m = np.floor(m)
    m = np.minimum(np.maximum(m, F32(-1024)), F32(1024))
    return m.astype(np.int32)


def align_rows_ref(img, a, b, c):
    """the image sampled at row y + dy(x, y): two rows blended in sixteenths, rows clamped to the image; bytes 0 .. 2 of a pixel"""
    H, W = img.shape[:2]
    q = field_q(H, W, a, b, c)
    y0 = np.arange(H, dtype=np.int32)[:, None] + (q >> 4)
    f = (q & 15)[:, :, None]
    r0 = np.clip(y0, 0, H - 1)
    r1 = np.clip(y0 + 1, 0, H - 1)
    cols = np.broadcast_to(np.arange(W)[None, :], (H, W))
    p0 = img[r0, cols, :3].astype(np.int32)
    p1 = img[r1, cols, :3].astype(np.int32)
    return (((16 - f) * p0 + f * p1 + 8) >> 4).astype(np.uint8)


def align_frame_ref(left, right, a, b, c):
    """the aligned pair as one side-by-side BGR frame: the left eye copied, the right eye through align_rows_ref"""
    return np.concatenate([left[:, :, :3], align_rows_ref(right, a, b, c)], axis=1)


# -------------------------------------------------------------------------------------------------------------- measure
def grey_of(img):
    """the project's grey_of: (u8)(b*c + g*c + r*c) in f32, c = 0.33333334f"""
    k = F32(0.33333334)
    b = img[..., 0].astype(F32) * k
    g = img[..., 1].astype(F32) * k
    r = img[..., 2].astype(F32) * k
    s = b + g
    s = s + r
    return s.astype(np.uint8)


def profiles_ref(img):
    """P[j][y] = the sum of grey over column band j of row y, KB x H uint32"""
    H, W = img.shape[:2]
    g = grey_of(img).astype(np.uint32)
    return np.stack([g[:, j * W // KB:(j + 1) * W // KB].sum(axis=1, dtype=np.uint32) for j in range(KB)])


def gradient_ref(P):
    H = P.shape[1]
    y = np.arange(H)
    return P[:, np.minimum(y + 1, H - 1)].astype(np.int64) - P[:, np.maximum(y - 1, 0)].astype(np.int64)


def sad_ref(PL, PR, R):
    """S[j][k][d + R] = sum over the rows of block k of |G_L[j][y] - G_R[j][clamp(y + d)]|, KB x KR x (2R+1) uint32"""
    H = PL.shape[1]
    GL, GR = gradient_ref(PL), gradient_ref(PR)
    S = np.zeros((KB, KR, 2 * R + 1), np.uint32)
    for k in range(KR):
        y = np.arange(k * H // KR, (k + 1) * H // KR)
        for d in range(-R, R + 1):
            yy = np.clip(y + d, 0, H - 1)
            S[:, k, d + R] = np.abs(GL[:, y] - GR[:, yy]).sum(axis=1).astype(np.uint32)
    return S


def blocks_ref(S, R):
    """per block (index i = j * KR + k): valid, offset o and weight w, both f64"""
    n = 2 * R + 1
    valid = np.zeros(KB * KR, bool)
    o = np.zeros(KB * KR, np.float64)
    w = np.zeros(KB * KR, np.float64)
    for j in range(KB):
        for k in range(KR):
            s = S[j, k].astype(np.int64)
            best, bi = int(s[R]), R
            for m in range(1, R + 1):  # d = 0, -1, +1, -2, +2, ...: strict less-than, ties go to the smaller |d|
                for i in (R - m, R + m):
                    if int(s[i]) < best:
                        best, bi = int(s[i]), i
            if bi == 0 or bi == n - 1:
                continue
            den = int(s[bi - 1]) - 2 * int(s[bi]) + int(s[bi + 1])
            if den <= 0:
                continue
            i = j * KR + k
            valid[i] = True
            num = np.float64(int(s[bi - 1]) - int(s[bi + 1]))
            t = num / np.float64(den)
            t = np.float64(0.5) * t
            o[i] = np.float64(bi - R) + t
            tot = max(1, int(s.sum()))
            t = np.float64(den) * np.float64(n)
            w[i] = t / np.float64(tot)
    return valid, o, w


def block_centres(H, W):
    """u_c, v_c of block i = j * KR + k: the centre of the band's columns and of the block's rows, relative to the frame's centre"""
    uc = np.zeros(KB * KR, np.float64)
    vc = np.zeros(KB * KR, np.float64)
    for j in range(KB):
        for k in range(KR):
            x0, x1 = j * W // KB, (j + 1) * W // KB
            y0, y1 = k * H // KR, (k + 1) * H // KR
            t = np.float64(x0 + x1 - 1) * np.float64(0.5)
            uc[j * KR + k] = t - np.float64(W - 1) * np.float64(0.5)
            t = np.float64(y0 + y1 - 1) * np.float64(0.5)
            vc[j * KR + k] = t - np.float64(H - 1) * np.float64(0.5)
    return uc, vc


DET_EPS = np.float64(1.0e-6)  # the determinant must exceed this share of the product of the diagonal (its upper bound)


def solve_ref(wt, o, uc, vc):
    """the weighted least-squares plane through the blocks of weight > 0, Cramer's rule in f64 with one operation per line, the
    sums taken in block order; fewer than 3 blocks or a determinant that is not clearly positive: b = c = 0, a = the weighted mean.
    None when no block has weight."""
    f = np.float64
    n = 0
    m00 = m01 = m02 = m11 = m12 = m22 = r0 = r1 = r2 = f(0.0)
    for i in range(len(wt)):
        if not wt[i] > 0.0:
            continue
        n += 1
        wi, u, v, oi = f(wt[i]), f(uc[i]), f(vc[i]), f(o[i])
        wu = wi * u
        wv = wi * v
        m00 = m00 + wi
        m01 = m01 + wu
        m02 = m02 + wv
        t = wu * u
        m11 = m11 + t
        t = wu * v
        m12 = m12 + t
        t = wv * v
        m22 = m22 + t
        t = wi * oi
        r0 = r0 + t
        t = wu * oi
        r1 = r1 + t
        t = wv * oi
        r2 = r2 + t
    if n == 0:
        return None
    # cofactors of the symmetric matrix [[m00 m01 m02] [m01 m11 m12] [m02 m12 m22]]
    t = m11 * m22
    p = m12 * m12
    c00 = t - p
    t = m01 * m22
    p = m12 * m02
    c01 = t - p
    t = m01 * m12
    p = m11 * m02
    c02 = t - p
    t = m00 * c00
    p = m01 * c01
    det = t - p
    p = m02 * c02
    det = det + p
    bound = m00 * m11
    bound = bound * m22
    bound = DET_EPS * bound
    if n < 3 or not det > bound:
        return (r0 / m00, f(0.0), f(0.0))
    t = m00 * m22
    p = m02 * m02
    c11 = t - p
    t = m00 * m12
    p = m01 * m02
    c12 = t - p
    t = m00 * m11
    p = m01 * m01
    c22 = t - p
    # x = adj(M) r / det; adj = [[c00 -c01 c02] [-c01 c11 -c12] [c02 -c12 c22]]
    t = c00 * r0
    p = c01 * r1
    t = t - p
    p = c02 * r2
    t = t + p
    a = t / det
    t = c11 * r1
    p = c01 * r0
    t = t - p
    p = c12 * r2
    t = t - p
    b = t / det
    t = c02 * r0
    p = c12 * r1
    t = t - p
    p = c22 * r2
    t = t + p
    c = t / det
    return (a, b, c)


def fit_ref(S, R, H, W):
    """steps 4 - 5: (a, b, c) in f64 and the number of valid blocks; None and 0 when no block is valid"""
    valid, o, w = blocks_ref(S, R)
    uc, vc = block_centres(H, W)
    x = solve_ref(w, o, uc, vc)
    if x is None:
        return None, 0
    w2 = w.copy()
    for i in range(len(w)):
        if not w[i] > 0.0:
            continue
        t = x[1] * uc[i]
        e = x[0] + t
        t = x[2] * vc[i]
        e = e + t
        e = o[i] - e
        if abs(e) > 1.0:
            w2[i] = 0.0
    y = solve_ref(w2, o, uc, vc)
    return (y if y is not None else x), int(valid.sum())


def state_update_ref(state, fit, rate, fresh=False):
    """step 6 on the four floats {valid, a, b, c}: returns the new state (float32 x 4)"""
    state = np.asarray(state, F32).copy()
    if fit is None:
        if fresh or state[0] == 0:
            state[:] = 0
        return state
    if fresh or state[0] == 0:
        return np.array([1.0, fit[0], fit[1], fit[2]], np.float64).astype(F32)
    for i in range(3):
        old = np.float64(state[1 + i])
        t = np.float64(fit[i]) - old
        t = np.float64(F32(rate)) * t
        state[1 + i] = F32(old + t)
    return state


def measure_ref(left, right, R, state=None, rate=1.0):
    """the whole measurement on two unpacked images: profiles (2 x KB x H), S, and the new state; state None = every frame on its own"""
    H, W = left.shape[:2]
    P = np.stack([profiles_ref(left), profiles_ref(right)])
    S = sad_ref(P[0], P[1], R)
    fit, nvalid = fit_ref(S, R, H, W)
    new = state_update_ref(np.zeros(4, F32) if state is None else state, fit, rate, fresh=state is None)
    return P, S, new, nvalid


# ------------------------------------------------------------------------------------------------- the statement's own checks
def _texture(H, W, seed):
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 256, size=(H // 3 + 2, W // 5 + 2, 3)).astype(np.float32)
    img = np.kron(base, np.ones((3, 5, 1), np.float32))[:H, :W] * 0.85 + rng.randint(0, 38, size=(H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def displace(img, a, b, c):
    """float bilinear resampling: out(y, x) = img(y - dy(x, y), x), so that the content of row y is found at row y + dy"""
    H, W = img.shape[:2]
    u = np.arange(W, dtype=np.float64)[None, :] - (W - 1) / 2.0
    v = np.arange(H, dtype=np.float64)[:, None] - (H - 1) / 2.0
    dy = a + b * u + c * v
    # the row of `out` at which content of source row s lands satisfies y = s + dy(x, y); sample the source at s = y - dy(x, y)
    s = np.arange(H, dtype=np.float64)[:, None] - dy
    s0 = np.floor(s)
    fr = (s - s0)[:, :, None]
    r0 = np.clip(s0.astype(np.int64), 0, H - 1)
    r1 = np.clip(s0.astype(np.int64) + 1, 0, H - 1)
    cols = np.broadcast_to(np.arange(W)[None, :], (H, W))
    p = (1.0 - fr) * img[r0, cols].astype(np.float64) + fr * img[r1, cols].astype(np.float64)
    return np.clip(np.floor(p + 0.5), 0, 255).astype(np.uint8)


def test_zero_field_is_the_identity():
    img = _texture(19, 23, 1)
    assert np.array_equal(align_rows_ref(img, 0.0, 0.0, 0.0), img)
    assert (field_q(19, 23, 0.0, 0.0, 0.0) == 0).all()


@pytest.mark.parametrize("n", [-40, -3, 1, 2, 7, 64, 100])
def test_integer_field_is_a_row_shift_with_clamped_ends(n):
    H = 21
    img = _texture(H, 17, 2)
    rows = np.clip(np.arange(H) + min(max(n, -64), 64), 0, H - 1)  # the field is clamped to +-64 rows
    assert np.array_equal(align_rows_ref(img, float(n), 0.0, 0.0), img[rows])


def test_fraction_blends_in_sixteenths():
    img = np.zeros((4, 1, 3), np.uint8)
    img[:, 0, 0] = [0, 160, 32, 255]
    out = align_rows_ref(img, 15.0 / 16.0, 0.0, 0.0)
    assert out[:, 0, 0].tolist() == [(1 * 0 + 15 * 160 + 8) >> 4, (160 + 15 * 32 + 8) >> 4, (32 + 15 * 255 + 8) >> 4, 255]


def test_flat_image_gives_no_valid_block():
    flat = np.full((40, 64, 3), 90, np.uint8)
    P, S, state, nvalid = measure_ref(flat, flat, 5)
    assert (S == 0).all() and nvalid == 0 and (state == 0).all()
    # a valid state is kept
    kept = state_update_ref(np.array([1, 2.5, 0.001, -0.002], F32), None, 0.5)
    assert kept.tolist() == np.array([1, 2.5, 0.001, -0.002], F32).tolist()


def test_ties_go_to_the_smaller_offset_and_negative_first():
    R = 3
    S = np.full((KB, KR, 2 * R + 1), 50, np.uint32)
    S[0, 0] = [50, 10, 30, 20, 30, 10, 50]   # minima at d = -2 and d = +2: -2 is scanned first
    S[1, 0] = [50, 10, 30, 10, 30, 40, 50]   # minima at d = -2 and d = 0: 0 wins
    S[2, 0] = [5, 10, 30, 40, 30, 40, 50]    # minimum at -R: not valid
    valid, o, w = blocks_ref(S, R)
    assert valid[0 * KR] and o[0 * KR] == -2.0 + 0.5 * (50 - 30) / (50 - 20 + 30)
    assert valid[1 * KR] and o[1 * KR] == 0.0
    assert not valid[2 * KR]
    assert valid.sum() == 2  # the flat blocks have den == 0


def test_fewer_than_three_blocks_fall_back_to_the_weighted_mean():
    R = 3
    S = np.full((KB, KR, 2 * R + 1), 50, np.uint32)
    S[0, 0] = [50, 40, 30, 10, 30, 40, 50]  # o = 0, den = 40
    S[5, 2] = [50, 40, 30, 20, 0, 40, 50]   # d = 1: o = 1 + 0.5 (20 - 40) / 60, den = 60
    fit, nvalid = fit_ref(S, R, 40, 64)
    valid, o, w = blocks_ref(S, R)
    assert nvalid == 2 and fit[1] == 0.0 and fit[2] == 0.0
    i, k = 0, 5 * KR + 2
    assert abs(fit[0] - (w[i] * o[i] + w[k] * o[k]) / (w[i] + w[k])) < 1e-12
    # blocks of one band only: three of them, but no plane is determined
    S = np.full((KB, KR, 2 * R + 1), 50, np.uint32)
    for k in range(3):
        S[3, k] = [50, 40, 30, 10, 30, 40, 50]
    fit, nvalid = fit_ref(S, R, 40, 64)
    assert nvalid == 3 and fit == (0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------------------ recovery
PAIRS = [("bud_2.bmp", "bud_3.bmp"), ("fish_1.bmp", "fish_2.bmp")]
FIELDS = [(0.0, 0.0, 0.0), (3.3, 0.0, 0.0), (-5.6, 0.004, 0.0), (2.2, -0.006, 0.01), (9.5, 0.002, -0.008), (0.4, 0.0, 0.0)]
_profiles = {}


def _pair(names):
    from stm_amd import bmp_io
    if names not in _profiles:
        _profiles[names] = tuple(bmp_io.read_bmp(os.path.join(GOLDEN, n)) for n in names)
    return _profiles[names]


def corner_errors(H, W, got, want):
    e = []
    for y in (0, H - 1):
        for x in (0, W - 1):
            u, v = x - (W - 1) / 2.0, y - (H - 1) / 2.0
            e.append(abs((got[0] + got[1] * u + got[2] * v) - (want[0] + want[1] * u + want[2] * v)))
    return e


@pytest.mark.parametrize("names", PAIRS, ids=["bud", "fish"])
@pytest.mark.parametrize("field", FIELDS)
def test_recovery_of_a_known_field(names, field):
    """the right eye displaced by a known field, R = 16: the fitted field is within 0.5 px (half a row: the census window still
    overlaps its match) of the true one at all four corners"""
    left, right = _pair(names)
    H, W = left.shape[:2]
    moved = displace(right, *field)
    P, S, state, nvalid = measure_ref(left, moved, 16)
    assert state[0] == 1.0 and nvalid >= 3
    err = corner_errors(H, W, [float(s) for s in state[1:]], field)
    print("field", field, "fit", state[1:].tolist(), "valid", nvalid, "corner errors", ["%.3f" % e for e in err])
    assert max(err) <= 0.5, (err, state)
