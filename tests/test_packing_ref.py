"""Packed stereo frames: the numpy statement of the unpacking that include/stm_hip.h defines (stm_demux_packed,
stm_demux_nv12_packed), tied to a plain scalar loop and to known answers.  tests/test_gpu_packing.py compares the library with
unpack_ref / unpack_nv12_ref bit for bit."""
import itertools

import numpy as np
import pytest

from test_nv12_ref import nv12_to_bgr_ref, random_planes

WEIGHTS = {0: (0, 96, 32, 0), 1: (-9, 111, 29, -3)}  # filter -> (w0, w1, w2, w3): the literal values of include/stm_hip.h
# every legal (packing, swap, filter)
SETTINGS = [(pk, sw, fl) for pk in range(4) for sw in (0, 1) for fl in ((0, 1) if pk & 1 else (0,))]


def packed_eye_shape(H, W, packing):
    """(Hp, Wp) of the table in stm_hip.h"""
    return (H, W // 2) if packing == 1 else (H // 2, W) if packing == 3 else (H, W)


def frame_shape(H, W, packing, gap):
    """(rows_f, the least row length) of the table in stm_hip.h"""
    Hp, Wp = packed_eye_shape(H, W, packing)
    return (H if packing < 2 else 2 * Hp + gap), (2 * Wp + gap if packing < 2 else W)


def eye_origin(e, H, W, packing, swap, gap):
    Hp, Wp = packed_eye_shape(H, W, packing)
    q = e ^ swap
    return (0, q * (Wp + gap)) if packing < 2 else (q * (Hp + gap), 0)


def expand2(P, axis, filt):
    """The expansion by two of stm_hip.h along `axis` of the uint8 array P (n samples there): int32 throughout, >> numpy's arithmetic
    shift, indices clamped to [0, n - 1]."""
    P = np.moveaxis(P.astype(np.int32), axis, 0)
    n = P.shape[0]
    x = np.arange(2 * n)
    k, s = x >> 1, np.where(x & 1, 1, -1)
    w0, w1, w2, w3 = (np.int32(w) for w in WEIGHTS[filt])
    tap = lambda i: P[np.clip(i, 0, n - 1)]  # noqa: E731
    acc = w0 * tap(k - s) + w1 * tap(k) + w2 * tap(k + s) + w3 * tap(k + 2 * s) + np.int32(64)
    assert acc.dtype == np.int32
    return np.moveaxis(np.clip(acc >> 7, 0, 255).astype(np.uint8), 0, axis)


def unpack_ref(frame, H, W, setting, gap=0):
    """The two unpacked eyes uint8 [H][W][3] of the packed BGR frame uint8 [>= rows_f][>= the least row length][>= 3];
    setting = (packing, swap, filter)"""
    packing, swap, filt = setting
    assert 0 <= packing <= 3 and swap in (0, 1) and filt in (0, 1) and gap >= 0 and (filt == 0 or packing & 1)
    assert not (packing == 1 and W % 2) and not (packing == 3 and H % 2)
    rows_f, need = frame_shape(H, W, packing, gap)
    assert frame.shape[0] >= rows_f and frame.shape[1] >= need
    Hp, Wp = packed_eye_shape(H, W, packing)
    out = []
    for e in (0, 1):
        r0, c0 = eye_origin(e, H, W, packing, swap, gap)
        P = frame[r0:r0 + Hp, c0:c0 + Wp, :3]
        out.append(np.ascontiguousarray(P) if not packing & 1 else expand2(P, 1 if packing == 1 else 0, filt))
        assert out[-1].shape == (H, W, 3)
    return out


def unpack_loop(frame, H, W, setting, gap=0):
    """the same, pixel by pixel in Python integers (// 128 is the floor the arithmetic shift takes)"""
    packing, swap, filt = setting
    Hp, Wp = packed_eye_shape(H, W, packing)
    w = WEIGHTS[filt]
    out = []
    for e in (0, 1):
        r0, c0 = eye_origin(e, H, W, packing, swap, gap)
        img = np.zeros((H, W, 3), np.uint8)
        for y in range(H):
            for x in range(W):
                for c in range(3):
                    if not packing & 1:
                        img[y, x, c] = frame[r0 + y, c0 + x, c]
                        continue
                    a, n = (x, Wp) if packing == 1 else (y, Hp)
                    k, s = a >> 1, (1 if a & 1 else -1)
                    acc = 64
                    for wt, i in zip(w, (k - s, k, k + s, k + 2 * s)):
                        i = min(max(i, 0), n - 1)
                        acc += wt * int(frame[r0 + y, c0 + i, c] if packing == 1 else frame[r0 + i, c0 + x, c])
                    img[y, x, c] = min(max(acc // 128, 0), 255)
        out.append(img)
    return out


def unpacked_sbs(frame, H, W, setting, gap=0):
    """the side-by-side frame [H][2W][3] whose halves are the two unpacked eyes: what a frame call under the packing computes on"""
    return np.ascontiguousarray(np.concatenate(unpack_ref(frame, H, W, setting, gap), axis=1))


def unpack_nv12_ref(y, uv, H, W, setting, gap=0, matrix=0):
    """stm_demux_nv12_packed: the unpacking of the BGR picture stm_demux_nv12's conversion gives on the packed frame"""
    packing = setting[0]
    assert H % 2 == 0 and W % 2 == 0 and gap % 2 == 0 and not (packing == 1 and W % 4) and not (packing == 3 and H % 4)
    return unpack_ref(nv12_to_bgr_ref(y, uv, matrix), H, W, setting, gap)


def build_frame(eyes, H, W, setting, gap=0, extra_cols=0, fill=None, seed=0):
    """a packed frame [rows_f][least row length + extra_cols][3] that holds the two PACKED eyes (eyes[e]: uint8 [Hp][Wp][3]);
    everything else -- the gap, the columns past the rule -- is `fill`, or noise if that is None"""
    packing, swap, _ = setting
    rows_f, need = frame_shape(H, W, packing, gap)
    Hp, Wp = packed_eye_shape(H, W, packing)
    shape = (rows_f, need + extra_cols, 3)
    frame = np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8) if fill is None else np.full(shape, fill, np.uint8)
    for e in (0, 1):
        r0, c0 = eye_origin(e, H, W, packing, swap, gap)
        frame[r0:r0 + Hp, c0:c0 + Wp] = eyes[e]
    return frame


def random_eyes(seed, H, W, packing):
    Hp, Wp = packed_eye_shape(H, W, packing)
    rng = np.random.RandomState(seed)
    eyes = [rng.randint(0, 256, size=(Hp, Wp, 3)).astype(np.uint8) for _ in (0, 1)]
    eyes[0][0, 0], eyes[1][-1, -1] = 0, 255
    return eyes


def squeeze2(img, axis):
    """2 : 1 by pair averaging ((a + b + 1) >> 1) along axis: how the tools make a packed frame from a full pair"""
    a = np.moveaxis(img.astype(np.int32), axis, 0)
    return np.moveaxis(((a[0::2] + a[1::2] + 1) >> 1).astype(np.uint8), 0, axis)


# ----------------------------------------------------------------------------- the definition
def test_weights():
    """both sets sum to 128, and filter 1 is the Catmull-Rom kernel at 1/4, exactly"""
    t = 0.25
    cr = (-0.5 * t ** 3 + t ** 2 - 0.5 * t, 1.5 * t ** 3 - 2.5 * t ** 2 + 1, -1.5 * t ** 3 + 2 * t ** 2 + 0.5 * t, 0.5 * t ** 3 - 0.5 * t ** 2)
    assert tuple(v * 128 for v in cr) == WEIGHTS[1]
    assert tuple(v * 128 for v in (0, 1 - t, t, 0)) == WEIGHTS[0]
    assert sum(WEIGHTS[0]) == 128 and sum(WEIGHTS[1]) == 128


@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("value", [0, 1, 127, 254, 255])
def test_constant_eye_comes_back_constant(value, filt):
    for n in (1, 2, 3, 8):
        assert (expand2(np.full((n, 3), value, np.uint8), 0, filt) == value).all()


@pytest.mark.parametrize("filt", [0, 1])
def test_step_at_every_alignment(filt):
    """a 0 | 255 step (and 255 | 0) at every position of eyes of 1 .. 7 samples, so that the clamp is taken on both sides, for
    both parities of the output index: the vector form against the weights written out by hand"""
    w = WEIGHTS[filt]
    both_sides = set()
    for n in range(1, 8):
        for edge in range(0, n + 1):
            for lo, hi in ((0, 255), (255, 0)):
                P = np.array([lo] * edge + [hi] * (n - edge), np.uint8)
                got = expand2(P, 0, filt)
                assert got.shape == (2 * n,)
                for x in range(2 * n):
                    k, s = x >> 1, (1 if x & 1 else -1)
                    idx = [k - s, k, k + s, k + 2 * s]
                    both_sides.update(("low", x & 1) for i in idx if i < 0)
                    both_sides.update(("high", x & 1) for i in idx if i > n - 1)
                    acc = 64 + sum(wt * int(P[min(max(i, 0), n - 1)]) for wt, i in zip(w, idx))
                    assert got[x] == min(max(acc >> 7, 0), 255), (n, edge, x)
    assert both_sides == {("low", 0), ("low", 1), ("high", 0), ("high", 1)}
    # known answers, worked by hand: the four samples around a step.  Filter 0: (32 * 255 + 64) >> 7 = 64, (96 * 255 + 64) >> 7 = 191.
    # Filter 1: ((29 - 3) * 255 + 64) >> 7 = 52, ((111 - 9) * 255 + 64) >> 7 = 203; the under- and overshoot beside them
    # ((-3 * 255 + 64) >> 7 = -6, (137 * 255 + 64) >> 7 = 273) are clipped
    P = np.array([0, 0, 255, 255], np.uint8)
    want = {0: [0, 0, 0, 64, 191, 255, 255, 255], 1: [0, 0, 0, 52, 203, 255, 255, 255]}[filt]
    assert expand2(P, 0, filt).tolist() == want


def test_filter_0_is_3a_plus_b():
    rng = np.random.RandomState(5)
    P = rng.randint(0, 256, size=(9,)).astype(np.uint8)
    got = expand2(P, 0, 0)
    for x in range(18):
        k, s = x >> 1, (1 if x & 1 else -1)
        a, b = int(P[k]), int(P[min(max(k + s, 0), 8)])
        assert got[x] == (3 * a + b + 2) >> 2
    # every pair of bytes
    a, b = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing="ij")
    assert np.array_equal((96 * a + 32 * b + 64) >> 7, (3 * a + b + 2) >> 2)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "p%d_s%d_f%d" % s)
@pytest.mark.parametrize("shape,gap", [((4, 6), 0), ((6, 10), 3), ((2, 2), 1)], ids=["4x6", "6x10_gap3", "2x2_gap1"])
def test_vectorised_form_is_the_scalar_loop(shape, gap, setting):
    H, W = shape
    frame = build_frame(random_eyes(H * 13 + W, H, W, setting[0]), H, W, setting, gap, extra_cols=2, seed=1)
    for a, b in zip(unpack_ref(frame, H, W, setting, gap), unpack_loop(frame, H, W, setting, gap)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("packing", [0, 2])
def test_full_packings_are_pure_copies(packing, swap):
    H, W, gap = 5, 7, 2
    eyes = random_eyes(3, H, W, packing)
    frame = build_frame(eyes, H, W, (packing, swap, 0), gap)
    l, r = unpack_ref(frame, H, W, (packing, swap, 0), gap)
    assert np.array_equal(l, eyes[0]) and np.array_equal(r, eyes[1])
    if packing == 0 and swap == 0:  # the reference's layout with a gap of 0
        frame = build_frame(eyes, H, W, (0, 0, 0), 0)
        assert np.array_equal(frame, np.concatenate(eyes, axis=1))


@pytest.mark.parametrize("setting", [s for s in SETTINGS if s[1] == 0], ids=lambda s: "p%d_f%d" % (s[0], s[2]))
def test_swap_exchanges_the_outputs(setting):
    H, W, gap = 6, 8, 4
    frame = build_frame(random_eyes(9, H, W, setting[0]), H, W, setting, gap)
    l, r = unpack_ref(frame, H, W, setting, gap)
    rs, ls = unpack_ref(frame, H, W, (setting[0], 1, setting[2]), gap)
    assert np.array_equal(l, ls) and np.array_equal(r, rs) and not np.array_equal(l, r)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "p%d_s%d_f%d" % s)
def test_the_gap_and_the_other_eye_never_reach_an_output(setting):
    """each eye alone, the rest of the frame (gap, other eye, columns past the rule) noise or zeros: the same eye comes out"""
    H, W, gap = 8, 12, 5
    eyes = random_eyes(17, H, W, setting[0])
    zero = np.zeros_like(eyes[0])
    noise = np.random.RandomState(2).randint(0, 256, size=zero.shape).astype(np.uint8)
    for e in (0, 1):
        a = build_frame([eyes[0] if e == 0 else zero, eyes[1] if e == 1 else zero], H, W, setting, gap, extra_cols=3, fill=0)
        b = build_frame([eyes[0] if e == 0 else noise, eyes[1] if e == 1 else noise], H, W, setting, gap, extra_cols=3, fill=None, seed=e)
        assert not np.array_equal(a, b)
        assert np.array_equal(unpack_ref(a, H, W, setting, gap)[e], unpack_ref(b, H, W, setting, gap)[e])


@pytest.mark.parametrize("matrix", [0, 3])
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "p%d_s%d_f%d" % s)
def test_nv12_equals_unpack_of_convert(setting, matrix):
    """chroma is replicated at PACKED resolution, in frame coordinates: the scalar loop on the converted frame, and, for the half
    packings, not the conversion of an unpacked NV12 frame"""
    H, W, gap = 8, 12, 2
    rows_f, need = frame_shape(H, W, setting[0], gap)
    y, uv = random_planes(H + W + matrix, rows_f, need + 2, need + 5, need + 8)
    got = unpack_nv12_ref(y, uv, H, W, setting, gap, matrix)
    want = unpack_loop(nv12_to_bgr_ref(y, uv, matrix), H, W, setting, gap)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # a chroma sample serves two packed columns / rows, so after a half unpacking four: the filter blends across that border
    r0, c0 = eye_origin(0, H, W, setting[0], setting[1], gap)
    assert r0 % 2 == 0 and c0 % 2 == 0


def test_geometry_table():
    assert [frame_shape(8, 12, p, 2) for p in range(4)] == [(8, 26), (8, 14), (18, 12), (10, 12)]
    assert [eye_origin(1, 8, 12, p, 0, 2) for p in range(4)] == [(0, 14), (0, 8), (10, 0), (6, 0)]
    assert [eye_origin(0, 8, 12, p, 1, 2) for p in range(4)] == [(0, 14), (0, 8), (10, 0), (6, 0)]
    assert all(eye_origin(0, 8, 12, p, 0, 2) == (0, 0) for p in range(4))
    assert len(SETTINGS) == 12 and len(set(SETTINGS)) == 12
    assert list(itertools.product((1, 3), (0, 1), (0, 1))) == [s for s in SETTINGS if s[0] & 1]


def test_squeeze_then_expand_keeps_a_constant():
    img = np.full((4, 8, 3), 77, np.uint8)
    for axis in (0, 1):
        for filt in (0, 1):
            assert (expand2(squeeze2(img, axis), axis, filt) == 77).all()


def test_frame_stream_geometry_helper():
    from stm_amd import video
    for p in range(4):
        rows_f, need = frame_shape(36, 132, p, 6)
        assert video.packed_frame_geometry(36, 132, (p, 1, 0, 6)) == (need, rows_f)
