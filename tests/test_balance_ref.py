"""The colour balance between the eyes (stm_set_balance, stm_balance_fit, stm_balance_apply; include/stm_hip.h has the definition line
by line) as a numpy statement, and the statement's own checks (no GPU).  tests/test_gpu_balance.py compares the kernels with it
bit for bit; tools/balance_effect.py measures with it what the balance buys the matcher."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

RADIUS = 8  # the smoothing window is +-8 levels, fixed
I64 = np.int64


# ---------------------------------------------------------------------------------------------------------------- the statement
def hist_ref(left, right):
    """step 1: h[e][c][v] over every pixel of eye e (0 = left), int64 (2, 3, 256); bytes of a pixel past the third are ignored"""
    h = np.zeros((2, 3, 256), I64)
    for e, img in enumerate((left, right)):
        for c in range(3):
            h[e, c] = np.bincount(np.asarray(img)[:, :, c].ravel(), minlength=256)
    return h


def match_ref(h):
    """steps 2 - 3: m[c][v] = min{u : 2 C[0][c][u] >= 2 C[1][c][v] - h[1][c][v]}"""
    C = np.cumsum(h, axis=2)
    m = np.zeros((3, 256), I64)
    for c in range(3):
        target = 2 * C[1, c] - h[1, c]
        m[c] = np.searchsorted(2 * C[0, c], target, side="left")
    assert (m <= 255).all()
    return m


def smooth_ref(h, m):
    """step 4: the offsets weighted by the right eye's counts over +-8 levels; empty windows carry from below, else from above"""
    s = np.zeros((3, 256), I64)
    for c in range(3):
        w = h[1, c]
        off = m[c] - np.arange(256)
        have = np.zeros(256, bool)
        for v in range(256):
            lo, hi = max(v - RADIUS, 0), min(v + RADIUS, 255)
            den = int(w[lo:hi + 1].sum())
            num = int((w[lo:hi + 1] * off[lo:hi + 1]).sum())
            if den > 0:
                s[c, v] = (2 * num + den) // (2 * den)  # Python's floor division
                have[v] = True
        assert have.any()
        first = int(np.argmax(have))
        for v in range(256):
            if not have[v]:
                s[c, v] = s[c, v - 1] if v > first else s[c, first]
    return s


def limit_ref(s, max_shift):
    """step 5: the clamp of the shift, the clamp of the level, the running maximum"""
    t = np.clip(np.arange(256) + np.clip(s, -max_shift, max_shift), 0, 255)
    return np.maximum.accumulate(t, axis=1)


def tables_ref(h, max_shift):
    """steps 2 - 5: t[c][v], int64 (3, 256)"""
    return limit_ref(smooth_ref(h, match_ref(h)), max_shift)


def rate_q_ref(rate):
    return int(min(max(int(np.floor(np.float32(rate) * np.float32(256.0) + np.float32(0.5))), 1), 256))


def update_ref(state, t, rate=1.0, fresh=False):
    """step 6: int32 state[769] = {valid, 3 x 256 levels in 1/256}; state None = no history"""
    x = 256 * np.asarray(t, I64).reshape(768)
    out = np.zeros(769, np.int32)
    out[0] = 1
    if state is None or fresh or int(state[0]) == 0:
        out[1:] = x
        return out
    old = np.asarray(state, np.int32)[1:].astype(I64)
    out[1:] = (old + ((rate_q_ref(rate) * (x - old) + 128) >> 8)).astype(np.int32)
    return out


def lut_ref(state):
    """step 7: the (3, 256) u8 tables of a state"""
    st = np.asarray(state, np.int32)[1:].astype(I64)
    return np.clip((st + 128) >> 8, 0, 255).astype(np.uint8).reshape(3, 256)


def fit_ref(left, right, max_shift=48, rate=1.0, state=None, fresh=False):
    """stm_balance_fit: (histograms, new state)"""
    assert left.shape[:2] == right.shape[:2] and left.shape[0] * left.shape[1] < 2 ** 31
    h = hist_ref(left, right)
    return h, update_ref(state, tables_ref(h, max_shift), rate, fresh)


def apply_ref(img, lut):
    """stm_balance_apply: the first three bytes of every pixel through the tables (B, G, R); (H, W, 3)"""
    lut = np.asarray(lut, np.uint8).reshape(3, 256)
    img = np.asarray(img)
    return np.stack([lut[c][img[:, :, c]] for c in range(3)], axis=2)


def balance_frame_ref(left, right, lut):
    """the pair as the frame calls take it under a balance: one side-by-side BGR frame, the left eye copied"""
    return np.ascontiguousarray(np.concatenate([np.asarray(left)[:, :, :3], apply_ref(right, lut)], axis=1))


def distort(img, gain, offset, gamma):
    """floor(255 (x/255)^gamma * gain + offset + 0.5) per channel in float64, clipped"""
    out = np.empty_like(img)
    x = np.arange(256, dtype=np.float64)
    for c in range(3):
        curve = np.clip(np.floor(255.0 * (x / 255.0) ** float(gamma[c]) * float(gain[c]) + float(offset[c]) + 0.5), 0, 255).astype(np.uint8)
        out[:, :, c] = curve[img[:, :, c]]
    return out


def _noise(H, W, seed, lo=0, hi=256):
    return np.random.RandomState(seed).randint(lo, hi, size=(H, W, 3)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- its own checks
@pytest.mark.parametrize("max_shift", [0, 5, 48, 255])
def test_equal_eyes_give_the_identity(max_shift):
    for img in (_noise(40, 64, 1), _noise(9, 7, 2, 90, 140), np.full((3, 5, 3), 17, np.uint8)):
        h = hist_ref(img, img)
        m = match_ref(h)
        occupied = h[1] > 0
        assert (m[occupied] == np.broadcast_to(np.arange(256), (3, 256))[occupied]).all()
        assert np.array_equal(tables_ref(h, max_shift), np.broadcast_to(np.arange(256), (3, 256)))


@pytest.mark.parametrize("max_shift", [0, 7, 20, 64, 255])
def test_flat_eyes_carry_in_both_directions(max_shift):
    left, right = np.full((6, 9, 3), 100, np.uint8), np.full((6, 9, 3), 120, np.uint8)
    t = tables_ref(hist_ref(left, right), max_shift)
    want = np.clip(np.arange(256) - min(20, max_shift), 0, 255)
    assert np.array_equal(t, np.broadcast_to(want, (3, 256)))


def test_two_occupied_levels():
    """right eye at 40 and 200 (one third / two thirds), left eye at 60 and 190: each level moves to its partner; the levels
    between carry from below, those under the first window from above"""
    right = np.full((3, 30, 3), 200, np.uint8)
    right[:, :10] = 40
    left = np.where(right == 40, 60, 190).astype(np.uint8)
    h = hist_ref(left, right)
    m = match_ref(h)
    assert (m[:, 40] == 60).all() and (m[:, 200] == 190).all()
    s = smooth_ref(h, m)
    assert (s[:, :49] == 20).all() and (s[:, 49:192] == 20).all() and (s[:, 192:209] == -10).all() and (s[:, 209:] == -10).all()
    t = tables_ref(h, 255)
    assert (t[:, 40] == 60).all() and (t[:, 200] == 211).all()  # 191 + 20 = 211 holds the running maximum over 192 .. 209 - 10
    assert (np.diff(t, axis=1) >= 0).all()
    lut = lut_ref(update_ref(None, tables_ref(h, 255)))
    assert np.array_equal(apply_ref(right[:, :10], lut), left[:, :10])


def test_max_shift_zero_is_the_identity():
    left, right = _noise(20, 30, 3), distort(_noise(20, 30, 3), (0.7,) * 3, (9,) * 3, (1.2,) * 3)
    assert np.array_equal(tables_ref(hist_ref(left, right), 0), np.broadcast_to(np.arange(256), (3, 256)))
    assert not np.array_equal(tables_ref(hist_ref(left, right), 48), np.broadcast_to(np.arange(256), (3, 256)))


def test_running_maximum_after_a_clamp():
    s = np.zeros((3, 256), I64)
    s[:, 100:110] = 30
    s[:, 110:] = -30
    s[:, :5] = -9
    t = limit_ref(s, 255)
    assert (t[:, :5] == 0).all() and (t[:, 109] == 139).all()
    assert (t[:, 110:170] == 139).all() and (t[:, 170] == 140).all()  # 139 is held until v - 30 passes it
    assert (limit_ref(s, 10)[:, 109] == 119).all() and (limit_ref(s, 10)[:, 110:130] == 119).all()
    s[:, 250:] = 40
    assert (limit_ref(s, 255)[:, 250:] == 255).all()


def test_floor_division_rounds_an_exact_negative_half_up():
    """one window holding two levels of equal weight with offsets -1 and -2: num / den = -1.5, which rounds to -1 (floor of -1.0),
    where C's truncating division of (2 num + den) / (2 den) = -2 / 2 ... = -4 / 4 would also have to be watched at -2.5 -> -2"""
    h = np.zeros((2, 3, 256), I64)
    h[1, :, 100] = 4
    h[1, :, 101] = 4
    for m_pair, want in (((99, 99), -2 + 1), ((98, 98), -2), ((97, 99), -3 + 1), ((101, 103), 2)):
        m = np.tile(np.arange(256), (3, 1)).astype(I64)
        m[:, 100], m[:, 101] = m_pair
        s = smooth_ref(h, m)
        num = (m_pair[0] - 100) + (m_pair[1] - 101)
        assert (s[:, 100] == want).all(), (m_pair, s[0, 100])
        assert want == int(np.floor(num / 2.0 + 0.5))
    assert (2 * -12 + 8) // (2 * 8) == -1 and int((2 * -12 + 8) / (2 * 8)) == -1
    assert (2 * -20 + 8) // (2 * 8) == -2 and int((2 * -20 + 8) / (2 * 8)) == -2
    assert (2 * -10 + 8) // (2 * 8) == -1 and int((2 * -10 + 8) / (2 * 8)) == 0  # where truncation would differ: -1.25 -> -1


def test_rate_q():
    assert [rate_q_ref(r) for r in (1.0, 0.5, 1.0 / 256, 1.0e-6, 0.999, 0.002)] == [256, 128, 1, 1, 256, 1]


@pytest.mark.parametrize("rate", [1.0, 0.5, 1.0 / 256])
def test_recursion_over_three_frames_keeps_the_table_monotone(rate):
    base = _noise(24, 40, 5)
    frames = [distort(base, (g,) * 3, (o,) * 3, (1.0,) * 3) for g, o in ((0.8, 0), (1.1, -12), (0.9, 20))]
    state = None
    states = []
    for k, right in enumerate(frames):
        h, state = fit_ref(base, right, 64, rate, state)
        states.append(state)
        assert state[0] == 1
        assert (np.diff(state[1:].reshape(3, 256), axis=1) >= 0).all(), k
        assert (np.diff(lut_ref(state).astype(int), axis=1) >= 0).all(), k
    t0, t1 = (256 * tables_ref(hist_ref(base, f), 64).reshape(768) for f in frames[:2])
    assert np.array_equal(states[0][1:], t0)  # no history: the tables themselves
    if rate == 1.0:
        assert np.array_equal(states[1][1:], t1)
    elif rate == 0.5:
        assert np.array_equal(states[1][1:], t0 + ((128 * (t1 - t0) + 128) >> 8))
        assert not np.array_equal(states[1][1:], t1)
    else:
        assert np.array_equal(states[1][1:], t0 + ((t1 - t0 + 128) >> 8))
        assert (np.abs(states[1][1:] - t0) <= np.abs(t1 - t0) // 256 + 1).all()
    _, again = fit_ref(base, frames[2], 64, rate, states[1], fresh=True)
    assert np.array_equal(again[1:], 256 * tables_ref(hist_ref(base, frames[2]), 64).reshape(768))


def test_step_7_rounding_and_clamp():
    st = np.zeros(769, np.int32)
    st[0] = 1
    st[1:9] = [0, 127, 128, 383, 384, 255 * 256 + 127, 255 * 256 + 128, 70000]
    st[9:12] = [-1, -129, -70000]
    lut = lut_ref(st).reshape(768)
    assert lut[:8].tolist() == [0, 0, 1, 1, 2, 255, 255, 255]
    assert lut[8:11].tolist() == [0, 0, 0]
    img = np.array([[[0, 1, 2, 9], [7, 255, 3, 9]]], np.uint8)
    table = np.arange(768).astype(np.uint8).reshape(3, 256)[:, ::-1]
    got = apply_ref(img, table)
    assert got.shape == (1, 2, 3) and got[0, 0].tolist() == [table[0, 0], table[1, 1], table[2, 2]]


# ---------------------------------------------------------------------------------------------------------------- recovery
PAIRS = [("bud_2.bmp", "bud_3.bmp"), ("fish_1.bmp", "fish_2.bmp")]
SETTINGS = [((1, 1, 1), (0, 0, 0), (1, 1, 1)),
            ((0.85, 0.85, 0.85), (0, 0, 0), (1, 1, 1)),
            ((1, 1, 1), (12, 12, 12), (1, 1, 1)),
            ((0.9, 1, 1.1), (6, 0, -8), (1, 1, 1)),
            ((1, 1, 1), (0, 0, 0), (1.25, 1.25, 1.25)),
            ((0.8, 0.95, 0.9), (10, -5, 4), (0.85, 1.1, 1.2))]
_pairs = {}


def _pair(names):
    from stm_amd import bmp_io
    if names not in _pairs:
        _pairs[names] = tuple(bmp_io.read_bmp(os.path.join(GOLDEN, n)) for n in names)
    return _pairs[names]


def recovery(left, right, setting, max_shift=64):
    """(mean absolute difference of the distorted right eye, of the matched right eye) against the undistorted one"""
    bad = distort(right, *setting)
    _, state = fit_ref(left, bad, max_shift)
    got = apply_ref(bad, lut_ref(state))
    ref = right.astype(np.int32)
    return float(np.abs(bad.astype(np.int32) - ref).mean()), float(np.abs(got.astype(np.int32) - ref).mean())


@pytest.mark.parametrize("k", range(len(SETTINGS)), ids=["setting%d" % (k + 1) for k in range(len(SETTINGS))])
@pytest.mark.parametrize("names", PAIRS, ids=["bud", "fish"])
def test_recovery_of_a_distorted_right_eye(stm, names, k):
    """Found (mean absolute difference in levels, distorted -> matched):
    bud   1: 0.0000 -> 0.3336   2:  9.0574 -> 0.4495   3: 11.8735 -> 0.4104   4: 2.6975 -> 0.6905   5: 11.5559 -> 1.0372
          6: 12.3741 -> 0.9475
    fish  1: 0.0000 -> 0.0000   2: 15.9723 -> 0.2517   3: 11.9781 -> 0.0195   4: 3.2423 -> 0.1084   5: 18.6266 -> 0.1176
          6: 14.9772 -> 0.2635"""
    left, right = _pair(names)
    before, after = recovery(left, right, SETTINGS[k])
    print("%s setting %d: %.4f -> %.4f" % (names[0], k + 1, before, after))
    assert after <= 2.0, (names, k + 1, before, after)
    if k == 0:
        assert before == 0.0 and after <= 0.5
