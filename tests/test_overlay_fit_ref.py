"""Overlay depth placement (stm_overlay_fit, stm_set_overlay_auto): the numpy statement of the definition in include/stm_hip.h that
the GPU tests (test_gpu_overlay_fit.py) compare against bit for bit, a scalar twin in Python's own arithmetic that keeps the
vectorised statement honest, and the fit's known answers.  No GPU."""
import math
import struct

import numpy as np
import pytest

from test_overlay_ref import overlay_ref, random_overlay

f32 = np.float32
NAN = float("nan")

# near_permille, margin, pad, limit_lo, limit_hi, rate_near, rate_far
P0 = dict(near_permille=0, margin=0.0, pad=0, limit_lo=-4096.0, limit_hi=4096.0, rate_near=1.0, rate_far=1.0)


def bits(state):
    return np.asarray(state, f32).tobytes()


# ----------------------------------------------------------------------------- the definition
def alpha_box_ref(overlay):
    """(r0, r1, q0, q1), inclusive, of the pixels with A != 0, or None"""
    on = np.asarray(overlay)[..., 3] != 0
    if not on.any():
        return None
    rows, cols = np.nonzero(on.any(axis=1))[0], np.nonzero(on.any(axis=0))[0]
    return int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])


def footprint_ref(box, x0, y0, pad, Hv, Wv, H, W):
    """the map rectangle (my0, my1, mx0, mx1), half open, or None"""
    if box is None:
        return None
    r0, r1, q0, q1 = box
    ya, yb = max(y0 + r0 - pad, 0), min(y0 + r1 + 1 + pad, Hv)
    xa, xb = max(x0 + q0 - pad, 0), min(x0 + q1 + 1 + pad, Wv)
    if ya >= yb or xa >= xb:
        return None
    return ya * H // Hv, (yb * H + Hv - 1) // Hv, xa * W // Wv, (xb * W + Wv - 1) // Wv


def fit_bins_ref(d):
    """stm_depth_fit's binning line on the values that are not NaN"""
    d = np.asarray(d, f32).ravel()
    d = d[~np.isnan(d)]
    with np.errstate(all="ignore"):
        v = (d * f32(4)).astype(f32)
        v = np.fmin(np.fmax(v, f32(-2048)), f32(2047))
        return np.floor((v + f32(0.5)).astype(f32)).astype(np.int64) + 2048


def _clamp(v, lo, hi):
    """min(max(v, lo), hi) as C's fmin(fmax(v, lo), hi): a NaN becomes lo"""
    v = lo if v != v else max(v, lo)
    return min(v, hi)


def _update(state, lo_bin, gain, conv, Wv, W, margin, limit_lo, limit_hi, rate_near, rate_far, fresh):
    """steps 4 (its last line) to 6 in Python floats, which are C doubles: one operation per line"""
    g, c = float(f32(gain)), float(f32(conv))
    margin, limit_lo, limit_hi = float(f32(margin)), float(f32(limit_lo)), float(f32(limit_hi))
    dp = (lo_bin - 2048) * 0.25
    e = g * dp
    e = e - c
    e = e * float(Wv)
    e = e / float(W)
    t = e - margin
    t = _clamp(t, limit_lo, limit_hi)
    if fresh or float(state[0]) == 0.0:
        d = t
    else:
        d_old = float(state[1])
        r = float(f32(rate_near)) if t < d_old else float(f32(rate_far))
        u = t - d_old
        u = r * u
        d = d_old + u
        d = _clamp(d, limit_lo, limit_hi)
    return np.array([1.0, f32(d), f32(e), 0.0], f32)


def overlay_fit_ref(dl, dr, overlay, x0, y0, Hv, Wv, gain=1.0, conv=0.0, near_permille=20, margin=1.0, pad=8, limit_lo=-4096.0,
                    limit_hi=4096.0, rate_near=1.0, rate_far=0.1, restart=False, state=None, cut_flag=0):
    """stm_overlay_fit: the new state (float32 [4]) from the maps, the overlay and the old state; n == 0 returns the old state's bits"""
    state = np.zeros(4, f32) if state is None else np.array(state, f32)
    dl, dr = np.asarray(dl, f32), np.asarray(dr, f32)
    H, W = dl.shape
    rect = footprint_ref(alpha_box_ref(overlay), int(x0), int(y0), int(pad), Hv, Wv, H, W)
    if rect is None:
        return state
    my0, my1, mx0, mx1 = rect
    b = np.concatenate([fit_bins_ref(dl[my0:my1, mx0:mx1]), fit_bins_ref(dr[my0:my1, mx0:mx1])])
    n = int(b.size)
    if n == 0:
        return state
    k = n * int(near_permille) // 1000
    cum = np.cumsum(np.bincount(b, minlength=4096))
    lo = int(np.argmax(cum > k))
    return _update(state, lo, gain, conv, Wv, W, margin, limit_lo, limit_hi, rate_near, rate_far, bool(restart) or cut_flag == 1)


def overlay_fit_scalar(dl, dr, overlay, x0, y0, Hv, Wv, gain=1.0, conv=0.0, near_permille=20, margin=1.0, pad=8, limit_lo=-4096.0,
                       limit_hi=4096.0, rate_near=1.0, rate_far=0.1, restart=False, state=None, cut_flag=0):
    """the same lines, one pixel at a time in Python's own arithmetic"""
    state = np.zeros(4, f32) if state is None else np.array(state, f32)
    H, W = len(dl), len(dl[0])
    r0 = r1 = q0 = q1 = None
    for r in range(len(overlay)):
        for q in range(len(overlay[0])):
            if int(overlay[r][q][3]) != 0:
                r0 = r if r0 is None else min(r0, r)
                r1 = r if r1 is None else max(r1, r)
                q0 = q if q0 is None else min(q0, q)
                q1 = q if q1 is None else max(q1, q)
    if r0 is None:
        return state
    ya, yb = max(y0 + r0 - pad, 0), min(y0 + r1 + 1 + pad, Hv)
    xa, xb = max(x0 + q0 - pad, 0), min(x0 + q1 + 1 + pad, Wv)
    if ya >= yb or xa >= xb:
        return state
    hist = [0] * 4096
    n = 0
    for y in range(ya * H // Hv, (yb * H + Hv - 1) // Hv):
        for x in range(xa * W // Wv, (xb * W + Wv - 1) // Wv):
            for m in (dl, dr):
                v = float(m[y][x])
                if v != v:
                    continue
                v = struct.unpack("f", struct.pack("f", 4.0 * v))[0] if abs(v) < 1e30 else math.copysign(math.inf, v)
                v = min(max(v, -2048.0), 2047.0)
                hist[int(math.floor(struct.unpack("f", struct.pack("f", v + 0.5))[0])) + 2048] += 1
                n += 1
    if n == 0:
        return state
    k = n * near_permille // 1000
    cum = 0
    for lo in range(4096):
        cum += hist[lo]
        if cum > k:
            break
    return _update(state, lo, gain, conv, Wv, W, margin, limit_lo, limit_hi, rate_near, rate_far, bool(restart) or cut_flag == 1)


def state_disparity_ref(state, limit_lo, limit_hi):
    """what the compositor reads from a state: fminf(fmaxf(state[1], limit_lo), limit_hi), a NaN going to limit_lo"""
    d = f32(np.asarray(state, f32)[1])
    d = f32(limit_lo) if np.isnan(d) else max(d, f32(limit_lo))
    return float(min(d, f32(limit_hi)))


def composite_from_state_ref(frame, overlay, x0, y0, state, limit_lo, limit_hi, shift, coords=None):
    return overlay_ref(frame, overlay, x0, y0, state_disparity_ref(state, limit_lo, limit_hi), shift, coords)


# ----------------------------------------------------------------------------- helpers of the tests
def strip(rows, cols, q0, q1, r0=0, r1=None, alpha=255):
    """a transparent overlay with an opaque block of columns q0 .. q1 and rows r0 .. r1 (inclusive)"""
    ov = np.zeros((rows, cols, 4), np.uint8)
    ov[r0:(rows if r1 is None else r1 + 1), q0:q1 + 1] = (alpha, alpha, alpha, alpha)
    return ov


def flat(H, W, v):
    return np.full((H, W), v, f32)


# ----------------------------------------------------------------------------- known answers
def test_a_fronto_parallel_pair():
    """delta = 8 everywhere, budget (0.5, 2), Wv = 2 W, margin 1: (0.5 * 8 - 2) * 2 - 1 = 3, and `nearest` is 4"""
    H, W = 20, 30
    st = overlay_fit_ref(flat(H, W, 8), flat(H, W, 8), strip(4, 20, 0, 19), 5, 10, 2 * H, 2 * W, gain=0.5, conv=2.0, margin=1.0)
    assert bits(st) == bits([1, 3, 4, 0])


def test_only_the_alpha_box_counts():
    """a nearer object under the transparent end of a full-width strip does not move the result; under the text it does"""
    H, W = 24, 64
    dl, dr = flat(H, W, 6), flat(H, W, 6)
    dl[18:, 50:] = -9  # near: smaller delta
    ov = strip(4, 64, 4, 20)  # text on the left, the right end empty
    kw = dict(P0, pad=2)
    assert bits(overlay_fit_ref(dl, dr, ov, 0, 18, H, W, **kw)) == bits([1, 6, 6, 0])
    assert bits(overlay_fit_ref(dl, dr, strip(4, 64, 4, 47), 0, 18, H, W, **kw)) == bits([1, 6, 6, 0])  # columns .. 49 with the pad
    assert bits(overlay_fit_ref(dl, dr, strip(4, 64, 4, 48), 0, 18, H, W, **kw)) == bits([1, -9, -9, 0])  # column 50 is reached


def test_the_near_percentile():
    """fewer than near_permille of nearer pixels are ignored, one more is not: n = 2 * 10 * 50 = 1000, k = 20"""
    H, W = 10, 50
    ov = strip(10, 50, 0, 49)
    for nearer, want in ((20, 5.0), (21, -3.0)):
        dl, dr = flat(H, W, 5), flat(H, W, 5)
        dl.ravel()[:nearer] = -3
        st = overlay_fit_ref(dl, dr, ov, 0, 0, H, W, **dict(P0, near_permille=20))
        assert bits(st) == bits([1, want, want, 0]), nearer


def test_both_clamps():
    H, W = 8, 8
    ov = strip(2, 2, 0, 1)
    for v, want in ((40.0, 10.0), (-40.0, -6.5)):
        st = overlay_fit_ref(flat(H, W, v), flat(H, W, v), ov, 1, 1, H, W, **dict(P0, limit_lo=-6.5, limit_hi=10.0))
        assert bits(st) == bits([1, want, v, 0])  # `nearest` is not clamped
    # the recursion is clamped too: an old disparity outside new limits comes back inside
    st = overlay_fit_ref(flat(H, W, 2), flat(H, W, 2), ov, 1, 1, H, W, state=[1, 50, 0, 0],
                         **dict(P0, limit_lo=-6.5, limit_hi=10.0, rate_near=0.5, rate_far=0.5))
    assert bits(st) == bits([1, 10.0, 2, 0])


def test_two_rates_over_a_near_then_far_sequence():
    """the scene comes nearer: followed at once (rate_near 1); it recedes: followed at rate_far"""
    H, W = 8, 8
    ov = strip(2, 2, 0, 1)
    kw = dict(P0, rate_near=1.0, rate_far=0.25)
    st = None
    got = []
    for v in (4, -4, 4, 4):
        st = overlay_fit_ref(flat(H, W, v), flat(H, W, v), ov, 1, 1, H, W, state=st, **kw)
        got.append(float(st[1]))
    assert got == [4.0, -4.0, -2.0, -0.5]


def test_restart_and_the_cut_flag_drop_the_history():
    H, W = 8, 8
    ov = strip(2, 2, 0, 1)
    kw = dict(P0, rate_near=0.5, rate_far=0.5)
    old = [1, -4, -4, 0]
    assert bits(overlay_fit_ref(flat(H, W, 4), flat(H, W, 4), ov, 1, 1, H, W, state=old, **kw)) == bits([1, 0, 4, 0])
    assert bits(overlay_fit_ref(flat(H, W, 4), flat(H, W, 4), ov, 1, 1, H, W, state=old, restart=True, **kw)) == bits([1, 4, 4, 0])
    assert bits(overlay_fit_ref(flat(H, W, 4), flat(H, W, 4), ov, 1, 1, H, W, state=old, cut_flag=1, **kw)) == bits([1, 4, 4, 0])
    assert bits(overlay_fit_ref(flat(H, W, 4), flat(H, W, 4), ov, 1, 1, H, W, state=old, cut_flag=0, **kw)) == bits([1, 0, 4, 0])
    assert bits(overlay_fit_ref(flat(H, W, 4), flat(H, W, 4), ov, 1, 1, H, W, state=[0, -4, -4, 0], **kw)) == bits([1, 4, 4, 0])


def test_nothing_counted_leaves_the_states_bits_alone():
    H, W = 12, 16
    old = np.array([1, NAN, -0.0, 7], f32)  # bits a rewrite would not reproduce
    dl, dr = flat(H, W, 3), flat(H, W, 3)
    opaque = strip(3, 4, 0, 3)
    assert bits(overlay_fit_ref(dl, dr, np.zeros((3, 4, 4), np.uint8), 2, 2, H, W, state=old, **P0)) == bits(old)  # transparent
    for x0, y0 in ((-4, 2), (W, 2), (2, -3), (2, H)):  # off the view on each side
        assert bits(overlay_fit_ref(dl, dr, opaque, x0, y0, H, W, state=old, **P0)) == bits(old), (x0, y0)
    for x0, y0 in ((-3, 2), (W - 1, 2), (2, -2), (2, H - 1)):  # one pixel inside: counted
        assert bits(overlay_fit_ref(dl, dr, opaque, x0, y0, H, W, state=old, restart=True, **P0)) == bits([1, 3, 3, 0]), (x0, y0)
    # a NaN in the old state does not survive the recursion: fmax sends it to limit_lo
    assert bits(overlay_fit_ref(dl, dr, opaque, 2, 2, H, W, state=old, **dict(P0, limit_lo=-7.0))) == bits([1, -7, 3, 0])
    nl, nr = dl.copy(), dr.copy()
    nl[2:5, 2:6] = NAN
    nr[2:5, 2:6] = NAN
    assert bits(overlay_fit_ref(nl, nr, opaque, 2, 2, H, W, state=old, **P0)) == bits(old)  # an all-NaN footprint
    nr[4, 5] = 1.25  # one number: the NaNs do not pull the result to the near end
    assert bits(overlay_fit_ref(nl, nr, opaque, 2, 2, H, W, state=old, restart=True, **P0)) == bits([1, 1.25, 1.25, 0])


def test_a_non_integer_ratio_rounds_outwards_at_both_ends():
    """Hv = 7 over H = 5, Wv = 11 over W = 4: view rows [2, 4) are map rows [1, 3) (10 div 7, ceil(20 / 7)); view columns [3, 6)
    are map columns [1, 3) (12 div 11, ceil(24 / 11))"""
    assert footprint_ref((0, 1, 0, 2), 3, 2, 0, 7, 11, 5, 4) == (1, 3, 1, 3)
    dl = np.arange(20, dtype=f32).reshape(5, 4)
    dr = flat(5, 4, 100)
    st = overlay_fit_ref(dl, dr, strip(2, 3, 0, 2), 3, 2, 7, 11, **P0)
    assert bits(st) == bits([1, f32(5.0 * 11 / 4), f32(5.0 * 11 / 4), 0])  # the least value inside is dl[1][1] = 5
    st = overlay_fit_ref(dl, dr, strip(2, 3, 0, 2), 3, 2, 7, 11, **dict(P0, near_permille=499))
    assert float(st[2]) == float(f32(10.0 * 11 / 4))  # k = 3 of n = 8: 5, 6, 9, then 10


@pytest.mark.parametrize("seed", range(6))
def test_the_scalar_twin_agrees(seed):
    rng = np.random.RandomState(seed)
    H, W = int(rng.randint(3, 12)), int(rng.randint(3, 14))
    Hv, Wv = int(rng.randint(3, 20)), int(rng.randint(3, 24))
    dl = (rng.randint(-40, 40, size=(H, W)) * 0.375).astype(f32)
    dr = (rng.randint(-40, 40, size=(H, W)) * 0.375).astype(f32)
    dl.ravel()[rng.randint(0, H * W, 3)] = (NAN, np.inf, -3000.0)
    dr.ravel()[rng.randint(0, H * W, 3)] = (NAN, -np.inf, 3000.0)
    ov = random_overlay(seed, int(rng.randint(1, 6)), int(rng.randint(1, 9)))
    state = None
    for step in range(4):
        kw = dict(gain=float(rng.randint(0, 9)) / 4, conv=float(rng.randint(-8, 8)) / 2, near_permille=int(rng.randint(0, 500)),
                  margin=float(rng.randint(-4, 4)) / 2, pad=int(rng.randint(0, 4)), limit_lo=-12.5, limit_hi=9.25,
                  rate_near=float(rng.randint(1, 9)) / 8, rate_far=float(rng.randint(1, 9)) / 8, restart=step == 2, cut_flag=int(step == 3))
        x0, y0 = int(rng.randint(-4, Wv)), int(rng.randint(-3, Hv))
        a = overlay_fit_ref(dl, dr, ov, x0, y0, Hv, Wv, state=state, **kw)
        b = overlay_fit_scalar(dl, dr, ov, x0, y0, Hv, Wv, state=state, **kw)
        assert bits(a) == bits(b), (seed, step)
        state = a


def test_the_video_tool_refuses_a_malformed_overlay_auto_option(capsys, tmp_path):
    """--overlay-auto needs --overlay, two limits in order and either none or all five of the optional numbers, each in its range
    (usage and -1, before any frame is read)"""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("stm_video", os.path.join(ROOT, "tools", "stm_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    good = tmp_path / "good.npy"
    np.save(good, np.zeros((4, 4, 4), np.uint8))
    ov = ["--overlay", str(good), "1", "2", "0"]
    for tail in (["--overlay-auto", "-30", "10"], ov + ["--overlay-auto", "-30"], ov + ["--overlay-auto", "10", "-30"],
                 ov + ["--overlay-auto", "-30", "x"], ov + ["--overlay-auto", "-30", "10", "20", "1", "8"],
                 ov + ["--overlay-auto", "-30", "10", "500", "1", "8", "1", "0.1"], ov + ["--overlay-auto", "-30", "10", "20", "1", "8", "0", "0.1"],
                 ov + ["--overlay-auto", "-30", "10", "20", "1", "4097", "1", "0.1"], ov + ["--overlay-auto", "-5000", "10"],
                 ov + ["--overlay-auto", "-30", "10", "20.5", "1", "8", "1", "0.1"], ov + ["--overlay-auto", "-30", "10", "20", "1", "8", "1", "1.5"]):
        assert mod.main(["stm_video"] + ["x"] * 16 + tail) == -1, tail
        assert "--overlay-auto LO HI [NEAR MARGIN PAD RATE_NEAR RATE_FAR]" in capsys.readouterr().out


def test_the_composite_from_a_state_is_the_overlay_at_the_clamped_disparity(orc):
    from test_overlay_ref import ANGLE, _frame, subpixel_shift_ref
    Ho, Wo, N = 12, 20, 8
    frame, ov = _frame(5, Ho, Wo), random_overlay(6, 3, 7)
    shift = subpixel_shift_ref(orc, Ho, Wo, N, 3, ANGLE)
    for d, want in ((2.5, 2.5), (9.0, 4.0), (-9.0, -3.5), (NAN, -3.5), (np.inf, 4.0), (-np.inf, -3.5)):
        assert state_disparity_ref([1, d, 0, 0], -3.5, 4.0) == want
        got = composite_from_state_ref(frame, ov, 4, 3, [1, d, 0, 0], -3.5, 4.0, shift)
        assert np.array_equal(got, overlay_ref(frame, ov, 4, 3, want, shift)), d
    assert not np.array_equal(overlay_ref(frame, ov, 4, 3, 4.0, shift), overlay_ref(frame, ov, 4, 3, -3.5, shift))
