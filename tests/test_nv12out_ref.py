"""NV12 output: the numpy statement of the conversion that include/stm_hip.h defines (stm_mux_nv12, stm_set_output), tied to its
coefficients recomputed from Kr / Kb, to the header's known answers, to a plain scalar loop, to an independent statement of the chroma
in exact fractions and to the floating-point converter of synth.  tests/test_gpu_nv12out.py compares the library with
bgr_to_nv12_ref bit for bit.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from test_nv12_ref import nv12_to_bgr_ref

# matrix -> (yo, yr, yg, yb, h, ur, ug, vg, vb): the literal values of include/stm_hip.h
COEF = {0: (16, 16829, 33039, 6416, 28784, 9714, 19070, 24103, 4681),
        1: (16, 11966, 40254, 4064, 28784, 6596, 22188, 26145, 2639),
        2: (0, 19595, 38470, 7471, 32768, 11058, 21710, 27439, 5329),
        3: (0, 13933, 46871, 4732, 32768, 7509, 25259, 29763, 3005)}
KR_KB = {0: (0.299, 0.114), 1: (0.2126, 0.0722), 2: (0.299, 0.114), 3: (0.2126, 0.0722)}
# matrix, (B, G, R) of a uniform 2 x 2 block -> (Y, U, V)
KNOWN = [(0, (0, 0, 0), (16, 128, 128)), (0, (255, 255, 255), (235, 128, 128)), (0, (0, 0, 255), (81, 90, 240)),
         (0, (255, 0, 0), (41, 240, 110)), (0, (0, 255, 0), (145, 54, 34)), (2, (255, 0, 0), (29, 255, 107)), (3, (0, 255, 0), (182, 30, 12))]


def luma_unclipped(b, g, r, matrix):
    """int32 arrays (or scalars) in, the sum after the shift and before clip255 out"""
    yo, yr, yg, yb = COEF[matrix][:4]
    return (yr * r + yg * g + yb * b + (yo << 16) + 32768) >> 16


def chroma_unclipped(sb, sg, sr, matrix):
    """the block sums (int32) in, (U, V) after the shift and before clip255 out"""
    _, _, _, _, h, ur, ug, vg, vb = COEF[matrix]
    return ((h * sb - ug * sg - ur * sr + (128 << 18) + (1 << 17)) >> 18, (h * sr - vg * sg - vb * sb + (128 << 18) + (1 << 17)) >> 18)


def bgr_to_nv12_ref(img, matrix=0):
    """The NV12 picture of a BGR image uint8 [H][W][>= 3], H and W even: (y uint8 [H][W], uv uint8 [H / 2][W], U and V interleaved).
    int32 throughout, >> is numpy's arithmetic shift."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    assert H % 2 == 0 and W % 2 == 0 and H >= 2 and W >= 2
    b, g, r = (img[:, :, c].astype(np.int32) for c in range(3))
    y = luma_unclipped(b, g, r, matrix)
    assert y.dtype == np.int32
    sb, sg, sr = (c.reshape(H // 2, 2, W // 2, 2).sum(axis=(1, 3), dtype=np.int32) for c in (b, g, r))
    u, v = chroma_unclipped(sb, sg, sr, matrix)
    uv = np.empty((H // 2, W), np.uint8)
    uv[:, 0::2] = np.clip(u, 0, 255)
    uv[:, 1::2] = np.clip(v, 0, 255)
    return np.clip(y, 0, 255).astype(np.uint8), uv


def bgr_to_nv12_loop(img, matrix=0):
    """the same, sample by sample in Python integers (// 65536 is the floor the arithmetic shift takes)"""
    yo, yr, yg, yb, h, ur, ug, vg, vb = COEF[matrix]
    H, W = img.shape[:2]
    y = np.zeros((H, W), np.uint8)
    uv = np.zeros((H // 2, W), np.uint8)
    for yy in range(H):
        for x in range(W):
            B, G, R = (int(img[yy, x, c]) for c in range(3))
            t = yr * R + yg * G + yb * B + (yo << 16) + 32768
            assert 0 <= t <= 1 << 26
            y[yy, x] = min(max(t // 65536, 0), 255)
    for j in range(H // 2):
        for k in range(W // 2):
            SB, SG, SR = (sum(int(img[2 * j + dy, 2 * k + dx, c]) for dy in (0, 1) for dx in (0, 1)) for c in range(3))
            for i, t in enumerate((h * SB - ug * SG - ur * SR + (128 << 18) + (1 << 17), h * SR - vg * SG - vb * SB + (128 << 18) + (1 << 17))):
                assert abs(t) <= 1 << 26  # reached by full-range blue: U = 256 before its clip
                uv[j, 2 * k + i] = min(max(t // (1 << 18), 0), 255)
    return y, uv


def nv12_surface_ref(img, matrix, pitch=0, uv_row=0, fill=0):
    """the surface stm_set_output describes, uint8 [R + H / 2][P], with `fill` in every byte that is no sample"""
    H, W = img.shape[:2]
    P, R = pitch or W, uv_row or H
    y, uv = bgr_to_nv12_ref(img, matrix)
    s = np.full((R + H // 2, P), fill, np.uint8)
    s[:H, :W] = y
    s[R:, :W] = uv
    return s


def random_image(seed, H, W, E=3):
    """random pixels with black, white and the primaries in it (H * W >= 8 keeps them all)"""
    img = np.random.RandomState(seed).randint(0, 256, size=(H, W, E)).astype(np.uint8)
    flat = img.reshape(-1, E)
    for i, px in enumerate(((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255))[:len(flat)]):
        flat[i * (len(flat) // 5) % len(flat), :3] = px
    return img


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
def test_coefficients_recomputed_from_kr_kb(matrix):
    kr, kb = KR_KB[matrix]
    sy, sc, yo = (219.0 / 255.0, 224.0 / 255.0, 16) if matrix < 2 else (1.0, 1.0, 0)
    exact = dict(ys=65536 * sy, yr=65536 * kr * sy, yb=65536 * kb * sy, h=32768 * sc, ur=65536 * kr * sc / (2 * (1 - kb)),
                 vb=65536 * kb * sc / (2 * (1 - kr)))
    for name, v in exact.items():
        assert abs(v - np.floor(v) - 0.5) > 1e-6, name  # none is a tie
    k = {name: int(np.rint(v)) for name, v in exact.items()}
    got = (yo, k["yr"], k["ys"] - k["yr"] - k["yb"], k["yb"], k["h"], k["ur"], k["h"] - k["ur"], k["h"] - k["vb"], k["vb"])
    assert got == COEF[matrix]


def test_known_answers():
    for matrix, bgr, want in KNOWN:
        img = np.empty((2, 2, 3), np.uint8)
        img[:] = bgr
        y, uv = bgr_to_nv12_ref(img, matrix)
        assert (y == want[0]).all() and tuple(uv[0]) == want[1:], (matrix, bgr, y[0, 0], uv[0], want)
        yl, uvl = bgr_to_nv12_loop(img, matrix)
        assert np.array_equal(yl, y) and np.array_equal(uvl, uv)
    sb = np.int32(4 * 255)
    assert chroma_unclipped(sb, np.int32(0), np.int32(0), 2)[0] == 256  # the one clip: full-range blue


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
def test_every_grey_has_neutral_chroma_and_the_range_ends_are_met(matrix):
    g = np.arange(256, dtype=np.uint8)
    img = np.repeat(np.repeat(g[None, :, None], 2, axis=0), 2, axis=1)  # 2 x 512: each grey one 2 x 2 block
    img = np.repeat(img, 3, axis=2)
    y, uv = bgr_to_nv12_ref(img, matrix)
    assert (uv == 128).all()
    lo, hi = (16, 235) if matrix < 2 else (0, 255)
    assert y[0, 0] == lo and y[0, -1] == hi
    assert (np.diff(y[0].astype(int)) >= 0).all()


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(2, 2), (4, 6), (6, 10)], ids=lambda s: "%dx%d" % s)
def test_vectorised_form_is_the_scalar_loop(shape, matrix):
    img = random_image(shape[0] * 31 + shape[1] + matrix, shape[0], shape[1], 4)
    y, uv = bgr_to_nv12_ref(img, matrix)
    yl, uvl = bgr_to_nv12_loop(img, matrix)
    assert np.array_equal(y, yl) and np.array_equal(uv, uvl)


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
def test_exhaustive_cube_luma_never_clips(matrix):
    """all 2^24 (B, G, R): Y before its clip is already in [yo, 255 - (limited ? 20 : 0)], and no intermediate exceeds 2^26"""
    G, R = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing="ij")
    yo, yr, yg, yb = COEF[matrix][:4]
    lo, hi = (16, 235) if matrix < 2 else (0, 255)
    for B in range(256):
        t = yr * R + yg * G + yb * np.int32(B) + (yo << 16) + 32768
        assert t.min() >= 0 and t.max() <= 1 << 26
        y = luma_unclipped(np.int32(B), G, R, matrix)
        assert y.min() >= lo and y.max() <= hi


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
def test_chroma_range_over_the_block_sums_corners(matrix):
    """U and V are linear in the block sums, so their extremes lie at the corners of [0, 1020]^3: only U or V = 256 leaves [0, 255]"""
    for sb in (0, 1020):
        for sg in (0, 1020):
            for sr in (0, 1020):
                for t in chroma_unclipped(np.int32(sb), np.int32(sg), np.int32(sr), matrix):
                    assert 0 <= t <= 256


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
def test_chroma_is_the_exact_mean_of_the_pixels_chroma_rounded_once(matrix):
    """an independent statement in exact fractions: per-pixel chroma from the integer coefficients, the mean of four, floor(x + 1/2)"""
    _, _, _, _, h, ur, ug, vg, vb = COEF[matrix]
    rng = np.random.RandomState(40 + matrix)
    for _ in range(200):
        blk = rng.randint(0, 256, size=(2, 2, 3)).astype(np.uint8)
        if rng.randint(4) == 0:
            blk[:] = rng.choice([0, 255], size=(2, 2, 3))
        us = [Fraction(h * int(b) - ug * int(g) - ur * int(r), 65536) for b, g, r in blk.reshape(4, 3)]
        vs = [Fraction(h * int(r) - vg * int(g) - vb * int(b), 65536) for b, g, r in blk.reshape(4, 3)]
        want = [min(max((sum(c) / 4 + 128 + Fraction(1, 2)).__floor__(), 0), 255) for c in (us, vs)]
        _, uv = bgr_to_nv12_ref(blk, matrix)
        assert list(uv[0]) == want, (blk.tolist(), uv[0], want)


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
def test_against_the_floating_point_converter(matrix):
    """synth.bgr_to_nv12 (float64, round to nearest) on the synthetic frame: each integer coefficient is off by at most 0.5 / 65536, a
    derived one by at most 1 / 65536, so a sum of three is off by less than 255 * 2 / 65536 < 0.008 of a level, so what remains is one rounding: both planes differ by at most 1.
    The share of differing samples is printed, not bounded."""
    from stm_amd import synth
    sbs, _ = synth.sbs_frame(96, 160, 16, 8)
    y, uv = bgr_to_nv12_ref(sbs, matrix)
    yf, uvf = synth.bgr_to_nv12(sbs, matrix)
    dy, duv = np.abs(y.astype(int) - yf), np.abs(uv.astype(int) - uvf)
    print("matrix %d: Y differs in %.4f%% of the samples, UV in %.4f%%" % (matrix, 100.0 * (dy != 0).mean(), 100.0 * (duv != 0).mean()))
    assert dy.max() <= 1 and duv.max() <= 1


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
def test_round_trip_through_the_input_conversion(matrix):
    """bgr_to_nv12_ref followed by nv12_to_bgr_ref on the synthetic frame: measured and printed; asserted is only that it beats the
    frame whose chroma plane was zeroed (all 128), as test_bgr_to_nv12_round_trip does for the floating-point converter."""
    from stm_amd import synth
    sbs, _ = synth.sbs_frame(96, 160, 16, 8)
    y, uv = bgr_to_nv12_ref(sbs, matrix)
    err = np.abs(nv12_to_bgr_ref(y, uv, matrix).astype(np.int32) - sbs)
    grey = np.abs(nv12_to_bgr_ref(y, np.full_like(uv, 128), matrix).astype(np.int32) - sbs)
    print("matrix %d: max |error| %d, mean |error| %.4f (chroma zeroed: max %d, mean %.4f)"
          % (matrix, err.max(), err.mean(), grey.max(), grey.mean()))
    assert err.mean() < grey.mean()


def test_surface_layout():
    img = random_image(5, 4, 6)
    s = nv12_surface_ref(img, 1, pitch=9, uv_row=7, fill=200)
    y, uv = bgr_to_nv12_ref(img, 1)
    assert s.shape == (9, 9) and np.array_equal(s[:4, :6], y) and np.array_equal(s[7:, :6], uv)
    assert (s[:, 6:] == 200).all() and (s[4:7] == 200).all()
    assert np.array_equal(nv12_surface_ref(img, 1), np.concatenate([y, uv], axis=0))
