"""NV12 input: the numpy statement of the conversion that include/stm_hip.h defines (stm_demux_nv12), tied to a plain scalar loop,
to the coefficients recomputed from Kr / Kb and to the header's known answers, and the host helpers around it
(synth.bgr_to_nv12, video.read_nv12_sequence).  tests/test_gpu_nv12.py compares the library with nv12_to_bgr_ref bit for bit."""
import numpy as np
import pytest

# matrix -> (ky, rv, gu, gv, bu, yo): the literal values of include/stm_hip.h
COEF = {0: (76309, 104597, 25675, 53279, 132201, 16),
        1: (76309, 117489, 13975, 34925, 138438, 16),
        2: (65536, 91881, 22553, 46802, 116130, 0),
        3: (65536, 103206, 12276, 30679, 121609, 0)}
KR_KB = {0: (0.299, 0.114), 1: (0.2126, 0.0722), 2: (0.299, 0.114), 3: (0.2126, 0.0722)}
# (Y, U, V) -> (B, G, R), matrix 0
KNOWN = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((126, 128, 128), (128, 128, 128)),
         ((81, 90, 240), (0, 0, 254)), ((0, 0, 0), (0, 136, 0)), ((255, 255, 255), (255, 125, 255)), ((255, 0, 255), (20, 225, 255))]


def _unclipped(Y, U, V, matrix):
    """the three sums after the shift, before clip255; int32 arrays (or scalars) in, int32 out"""
    ky, rv, gu, gv, bu, yo = COEF[matrix]
    C, D, E = Y - yo, U - 128, V - 128
    return (ky * C + bu * D + 32768) >> 16, (ky * C - gu * D - gv * E + 32768) >> 16, (ky * C + rv * E + 32768) >> 16


def nv12_to_bgr_ref(y, uv, matrix=0):
    """The side-by-side BGR frame uint8 [H][Wsbs][3] of an NV12 frame: y uint8 [H][Wsbs], uv uint8 [H / 2][>= 2 * ((Wsbs + 1) / 2)]
    (any row strides), chroma replicated.  int32 throughout, >> is numpy's arithmetic shift."""
    H, Wsbs = y.shape
    assert H % 2 == 0 and uv.shape[0] == H // 2
    xs = np.arange(Wsbs)
    rows = np.arange(H) >> 1
    U = uv.astype(np.int32)[rows][:, 2 * (xs >> 1)]
    V = uv.astype(np.int32)[rows][:, 2 * (xs >> 1) + 1]
    b, g, r = _unclipped(y.astype(np.int32), U, V, matrix)
    assert b.dtype == np.int32
    return np.clip(np.stack([b, g, r], axis=2), 0, 255).astype(np.uint8)


def nv12_to_bgr_loop(y, uv, matrix=0):
    """the same, pixel by pixel in Python integers (// 65536 is the floor the arithmetic shift takes)"""
    ky, rv, gu, gv, bu, yo = COEF[matrix]
    H, Wsbs = y.shape
    out = np.zeros((H, Wsbs, 3), np.uint8)
    for yy in range(H):
        for x in range(Wsbs):
            C = int(y[yy, x]) - yo
            D = int(uv[yy >> 1, 2 * (x >> 1)]) - 128
            E = int(uv[yy >> 1, 2 * (x >> 1) + 1]) - 128
            for c, v in enumerate((ky * C + bu * D + 32768, ky * C - gu * D - gv * E + 32768, ky * C + rv * E + 32768)):
                assert abs(v) < 1 << 26
                out[yy, x, c] = min(max(v // 65536, 0), 255)
    return out


def nv12_halves(y, uv, W, matrix=0, elem_sz=3):
    """what stm_demux_nv12 returns: the two views [H][W][elem_sz], bytes past the third 0"""
    bgr = nv12_to_bgr_ref(y, uv, matrix)
    H = y.shape[0]
    out = []
    for x0 in (0, W):
        v = np.zeros((H, W, elem_sz), np.uint8)
        v[:, :, :3] = bgr[:, x0:x0 + W]
        out.append(v)
    return out


def random_planes(seed, H, Wsbs, pitch_y=None, pitch_uv=None):
    """random planes with 0 and 255 in each of Y, U and V; returned as views of pitched buffers (the padding holds other bytes)"""
    rng = np.random.RandomState(seed)
    pitch_y = pitch_y or Wsbs
    pitch_uv = pitch_uv or 2 * ((Wsbs + 1) // 2)
    yb = rng.randint(0, 256, size=(H, pitch_y)).astype(np.uint8)
    ub = rng.randint(0, 256, size=(H // 2, pitch_uv)).astype(np.uint8)
    y, uv = yb[:, :Wsbs], ub[:, :2 * ((Wsbs + 1) // 2)]
    y[0, 0], y[-1, -1] = 0, 255
    uv[0, 0], uv[0, 1], uv[-1, -2], uv[-1, -1] = 0, 255, 255, 0
    return y, uv


def nv12_frame(y, uv):
    """the [H * 3 / 2][Wsbs] array of a frame stream in NV12 mode: the Y plane, then the UV plane (Wsbs even)"""
    assert y.shape[1] % 2 == 0 and uv.shape == (y.shape[0] // 2, y.shape[1])
    return np.ascontiguousarray(np.concatenate([y, uv], axis=0))


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
def test_coefficients_recomputed_from_kr_kb(matrix):
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    ky, s, yo = (255.0 / 219.0, 255.0 / 224.0, 16) if matrix < 2 else (1.0, 1.0, 0)
    exact = (ky, 2 * (1 - kr) * s, 2 * kb * (1 - kb) * s / kg, 2 * kr * (1 - kr) * s / kg, 2 * (1 - kb) * s)
    for v in exact:
        assert abs(v * 65536 - np.floor(v * 65536) - 0.5) > 1e-6  # none is a tie
    assert tuple(int(np.rint(v * 65536)) for v in exact) + (yo,) == COEF[matrix]


def test_known_answers():
    for (Y, U, V), want in KNOWN:
        y = np.full((2, 2), Y, np.uint8)
        uv = np.array([[U, V]], np.uint8)
        got = nv12_to_bgr_ref(y, uv, 0)
        assert (got == np.array(want, np.uint8)).all(), ((Y, U, V), got[0, 0], want)
        assert np.array_equal(nv12_to_bgr_loop(y, uv, 0), got)


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(2, 2), (4, 6), (6, 9), (10, 14)], ids=lambda s: "%dx%d" % s)
def test_vectorised_form_is_the_scalar_loop(shape, matrix):
    H, Wsbs = shape
    y, uv = random_planes(H * 31 + Wsbs + matrix, H, Wsbs, Wsbs + 3, 2 * ((Wsbs + 1) // 2) + 5)
    assert np.array_equal(nv12_to_bgr_ref(y, uv, matrix), nv12_to_bgr_loop(y, uv, matrix))


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
def test_exhaustive_cube_stays_in_range_and_takes_every_clip(matrix):
    """all 256^3 (Y, U, V): no intermediate reaches 2^26, the clipped result is in [0, 255], and each channel clips at both ends"""
    U, V = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing="ij")
    ky, rv, gu, gv, bu, yo = COEF[matrix]
    low, high = np.zeros(3, bool), np.zeros(3, bool)
    for Y in range(256):
        C = np.int32(Y - yo)
        for t in (ky * C + bu * (U - 128) + 32768, ky * C - gu * (U - 128) - gv * (V - 128) + 32768, ky * C + rv * (V - 128) + 32768):
            assert np.abs(t).max() < 1 << 26
        for c, v in enumerate(_unclipped(np.int32(Y), U, V, matrix)):
            low[c] |= bool((v < 0).any())
            high[c] |= bool((v > 255).any())
    assert low.all() and high.all()


def test_chroma_is_replicated_over_each_2x2_block():
    y = np.full((4, 8), 120, np.uint8)
    uv = np.random.RandomState(3).randint(0, 256, size=(2, 8)).astype(np.uint8)
    bgr = nv12_to_bgr_ref(y, uv, 0)
    for dy in (0, 1):
        for dx in (0, 1):
            assert np.array_equal(bgr[dy::2, dx::2], bgr[0::2, 0::2])


# ----------------------------------------------------------------------------- the host helpers
def test_read_nv12_sequence(tmp_path):
    from stm_amd import video
    H, Wsbs = 4, 6
    frames = [nv12_frame(*random_planes(k, H, Wsbs)) for k in range(3)]
    path = tmp_path / "clip.yuv"
    path.write_bytes(b"".join(f.tobytes() for f in frames))
    got = list(video.read_nv12_sequence(str(path), H, Wsbs))
    assert len(got) == 3 and all(g.shape == (H * 3 // 2, Wsbs) and g.dtype == np.uint8 for g in got)
    assert all(np.array_equal(a, b) for a, b in zip(got, frames))
    path.write_bytes(frames[0].tobytes() + b"\x00" * 5)
    with pytest.raises(ValueError):
        list(video.read_nv12_sequence(str(path), H, Wsbs))
    empty = tmp_path / "empty.yuv"
    empty.write_bytes(b"")
    assert list(video.read_nv12_sequence(str(empty), H, Wsbs)) == []


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
def test_bgr_to_nv12_round_trip(matrix):
    """synth.bgr_to_nv12 followed by the reference, on the synthetic frame: the error is measured and printed, not bounded by a
    guess; what is asserted is its direction -- a frame whose chroma was kept is closer to the original than one whose chroma
    plane was zeroed (all 128).  Measured, 96 x 320 synthetic frame, over the four matrices: max |error| 14 to 16 and mean |error|
    0.82 to 0.87 with the chroma kept (the 2 x 2 chroma mean at colour edges), against max 60 to 69 and mean 15.4 to 15.6 with it
    zeroed."""
    from stm_amd import synth
    sbs, _ = synth.sbs_frame(96, 160, 16, 8)
    y, uv = synth.bgr_to_nv12(sbs, matrix)
    assert y.shape == (96, 320) and uv.shape == (48, 320) and y.dtype == np.uint8 and uv.dtype == np.uint8
    err = np.abs(nv12_to_bgr_ref(y, uv, matrix).astype(np.int32) - sbs)
    grey = np.abs(nv12_to_bgr_ref(y, np.full_like(uv, 128), matrix).astype(np.int32) - sbs)
    print("matrix %d: max |error| %d, mean |error| %.4f (chroma zeroed: max %d, mean %.4f)"
          % (matrix, err.max(), err.mean(), grey.max(), grey.mean()))
    assert err.mean() < grey.mean()
