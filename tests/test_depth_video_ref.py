"""The numpy statement of a frame stream's packed 2D-plus-depth video input (stm_stream_input_packed_depth; include/stm_depth_video.h
states steps 0 and A' to A''' line by line, DESIGN.md section 34 gives the reasons) and its known answers.  depth_video_ref is
composed of unpack_ref / unpack_nv12_ref (step 0), the new decode_video_ref (A' to A''') and eye_ref (B to E).  No GPU:
tests/test_gpu_depth_video.py compares the kernel with depth_video_ref bit for bit, and imports the scene from here."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from test_depth_input_ref import COUNTS, LIMITS, decode_ref, eye_ref, scene_disp
from test_packing_ref import eye_origin, frame_shape, packed_eye_shape, unpack_nv12_ref, unpack_ref

f32 = np.float32
VIDEO_COUNTS = ("gated_even", "gated_odd", "ungated_even", "ungated_odd", "clamped_first", "clamped_last", "below_16", "above_235")


def code_ref(P, rng):
    """step A': (c, M) of the samples P, int32"""
    c = np.asarray(P).astype(np.int32)
    return (np.clip(c, 16, 235) - 16, 219) if rng else (c, 255)


def decode_video_ref(P, packing, rng, dfilter, dgate, lo, hi):
    """Steps A' to A''' on the depth picture's own region P (uint8 [Hp][Wp], the Y or G samples).  Returns (disp_l float32 [H][W],
    counts): the pairs of a squeezed picture by gate and parity (whatever dfilter is), the two clamps, the samples range 1 clips."""
    assert rng in (0, 1) and dfilter in (0, 1) and 0 <= dgate <= 255 and (dfilter == 0 or packing & 1)
    c, M = code_ref(P, rng)
    n = dict.fromkeys(VIDEO_COUNTS, 0)
    n["below_16"], n["above_235"] = int((np.asarray(P) < 16).sum()), int((np.asarray(P) > 235).sum())
    if not packing & 1:
        v = 4 * c
    else:
        axis = 1 if packing == 1 else 0
        c = np.moveaxis(c, axis, 0)
        m = c.shape[0]
        a = np.arange(2 * m)
        k, s = a >> 1, np.where(a & 1, 1, -1)
        nb = np.clip(k + s, 0, m - 1)
        c0, c1 = c[k], c[nb]
        gated = np.abs(c0 - c1) <= np.int32(dgate)
        inner = (nb == k + s).reshape((-1,) + (1,) * (c.ndim - 1))  # a clamped neighbour is the sample itself: no pair
        odd = (a & 1).astype(bool).reshape(inner.shape)
        n["gated_even"], n["gated_odd"] = int((gated & inner & ~odd).sum()), int((gated & inner & odd).sum())
        n["ungated_even"], n["ungated_odd"] = int((~gated & inner & ~odd).sum()), int((~gated & inner & odd).sum())
        n["clamped_first"], n["clamped_last"] = int((k + s < 0).sum()) * c[0].size, int((k + s > m - 1).sum()) * c[0].size
        v = np.where(gated & bool(dfilter), 3 * c0 + c1, 4 * c0)
        v = np.moveaxis(v, 0, axis)
    assert v.dtype == np.int32
    q4 = f32((float(f32(hi)) - float(f32(lo))) / (4.0 * M))
    t = (v.astype(f32) * q4).astype(f32)
    return (f32(lo) + t).astype(f32), n


def split_frame(frame, fmt):
    """(the BGR frame or (y, uv), the plane the depth samples are read from) of a frame as a stream takes it"""
    if fmt == "nv12":
        rows_f = frame.shape[0] * 2 // 3
        return (frame[:rows_f], frame[rows_f:]), frame[:rows_f]
    return frame, frame[..., 1]


def depth_video_ref(frame, H, W, fmt, matrix, setting, gap, rng, dfilter, dgate, lo, hi, fill, gate):
    """The definition on a whole frame: BGR uint8 [rows_f][>= the least row length][>= 3], or NV12 uint8 [rows_f * 3 / 2][Wsbs];
    setting = (packing, swap, filter).  Returns (img_l, disp_l, img_r, disp_r, hole mask, counts)."""
    packing, swap, _ = setting
    src, samples = split_frame(frame, fmt)
    img = unpack_nv12_ref(src[0], src[1], H, W, setting, gap, matrix)[0] if fmt == "nv12" else unpack_ref(src, H, W, setting, gap)[0]
    Hp, Wp = packed_eye_shape(H, W, packing)
    r0, c0 = eye_origin(1, H, W, packing, swap, gap)
    disp_l, nd = decode_video_ref(samples[r0:r0 + Hp, c0:c0 + Wp], packing, rng, dfilter, dgate, lo, hi)
    img_r, disp_r, holes, n = eye_ref(img, disp_l, fill, gate)
    n.update(nd)
    return img, disp_l, img_r, disp_r, holes, n


def scene_codes(H, W, packing, rng, lo, hi, k=0):
    """The depth picture uint8 [Hp][Wp] of test_depth_input_ref's scene, frame k: its float map quantised between lo and hi to 0 ..
    255 (range 0) or 16 .. 235 (range 1), every second sample along a squeezed axis; with range 1 a sample below 16 and one above 235
    in the first and last row where the map is at its ends anyway."""
    d = scene_disp(H, W, k).astype(np.float64)
    M = 219 if rng else 255
    c = np.clip(np.floor((d - lo) / (hi - lo) * M + 0.5), 0, M).astype(np.int32) + (16 if rng else 0)
    if packing == 1:
        c = c[:, 0::2]
    elif packing == 3:
        c = c[0::2, :]
    c = c.astype(np.uint8)
    if rng:
        c[0, 0] = 3 if c[0, 0] == 16 else c[0, 0]
        c[0, -1] = 9
        c[-1, 1] = 250
    return c


def build_video_frame(H, W, fmt, setting, gap, codes, seed=0, extra_cols=0, elem_sz=3, image=None):
    """A packed frame that holds `codes` as the depth picture: noise everywhere else -- the image half, the gap, spare columns, the
    B and R bytes (BGR) or the chroma (NV12) of the depth picture, so that a read outside the definition's shows.  image: the packed
    image half uint8 [Hp][Wp][3] of a BGR frame, noise if None."""
    packing, swap, _ = setting
    rows_f, need = frame_shape(H, W, packing, gap)
    Hp, Wp = packed_eye_shape(H, W, packing)
    rs = np.random.RandomState(seed * 7919 + H * 131 + W)
    cols = need + extra_cols
    frame = rs.randint(0, 256, size=(rows_f * 3 // 2, cols) if fmt == "nv12" else (rows_f, cols, elem_sz)).astype(np.uint8)
    r0, c0 = eye_origin(1, H, W, packing, swap, gap)
    assert codes.shape == (Hp, Wp)
    if fmt == "nv12":
        frame[r0:r0 + Hp, c0:c0 + Wp] = codes
    else:
        frame[r0:r0 + Hp, c0:c0 + Wp, 1] = codes
        if image is not None:
            i0, j0 = eye_origin(0, H, W, packing, swap, gap)
            frame[i0:i0 + Hp, j0:j0 + Wp, :3] = image
    return frame


# ----------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("lo,hi", LIMITS)
def test_the_quarter_code_decode_is_the_u8_decode_of_depth_input(lo, hi):
    codes = np.arange(256, dtype=np.uint8).reshape(1, -1)
    for packing in (0, 2):
        got, _ = decode_video_ref(codes, packing, 0, 0, 0, lo, hi)
        assert got.dtype == f32 and np.array_equal(got.view(np.uint32), decode_ref(codes, "u8", lo, hi).view(np.uint32))
    got, _ = decode_video_ref(codes.T, 1, 0, 0, 0, lo, hi)  # one sample a row, replicated
    assert np.array_equal(got[:, 0].view(np.uint32), decode_ref(codes, "u8", lo, hi)[0].view(np.uint32)) and np.array_equal(got[:, 0], got[:, 1])


@pytest.mark.parametrize("lo,hi", [(-12.0, 12.0), (12.0, -12.0), (0.0, 64.0)])
def test_range_1_sends_16_to_lo_and_235_to_hi_and_clamps(lo, hi):
    P = np.array([[0, 3, 16, 17, 125, 234, 235, 236, 255]], np.uint8)
    d, n = decode_video_ref(P, 0, 1, 0, 0, lo, hi)
    assert d[0, 2] == f32(lo) and d[0, 0] == d[0, 1] == d[0, 2]
    assert abs(float(d[0, 6]) - hi) <= abs(hi - lo) * 2.0 ** -22 and d[0, 7] == d[0, 8] == d[0, 6]
    assert (np.diff(d[0, 2:7]) > 0).all() if hi > lo else (np.diff(d[0, 2:7]) < 0).all()
    assert n["below_16"] == 2 and n["above_235"] == 2


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
@pytest.mark.parametrize("shift", [4, -3])
def test_a_constant_depth_picture_shifts_the_image(fmt, shift):
    H, W = 4, 24
    lo, hi = -8.0, 8.0
    code = int(round((shift + (0.5 if shift > 0 else -0.5) - lo) / (hi - lo) * 255))  # decodes to the middle of the values that truncate to shift
    frame = build_video_frame(H, W, fmt, (0, 0, 0), 0, np.full((H, W), code, np.uint8), seed=3)
    img, dl, img_r, dr, holes, n = depth_video_ref(frame, H, W, fmt, 1, (0, 0, 0), 0, 0, 0, 0, lo, hi, 0, 0.0)
    assert (dl == dl[0, 0]).all() and int(dl[0, 0]) == shift and (dr == dl[0, 0]).all()
    a, b = max(shift, 0) + (shift < 0), W + min(shift, 0) - (shift > 0)
    assert np.array_equal(img_r[:, a:b], img[:, a - shift:b - shift])
    assert holes.any() and n["one_sided"] == H and n["two_sided"] == 0


def _expanded_pairs(P, axis):
    c = np.moveaxis(P.astype(np.int32), axis, 0)
    m = c.shape[0]
    a = np.arange(2 * m)
    k, s = a >> 1, np.where(a & 1, 1, -1)
    return c[k], c[np.clip(k + s, 0, m - 1)]


@pytest.mark.parametrize("packing", [1, 3])
def test_dfilter_1_is_dfilter_0_where_every_pair_is_beyond_the_gate(packing):
    rs = np.random.RandomState(packing)
    axis = 1 if packing == 1 else 0
    steps = np.array([0, 100, 30, 200, 60, 250, 10], np.int32).reshape((1, 7) if axis == 1 else (7, 1))  # neighbours at least 30 apart
    P = (steps + rs.randint(0, 3, size=(6, 7) if axis == 1 else (7, 6))).astype(np.uint8)
    assert (np.abs(np.diff(P.astype(np.int32), axis=axis)) > 5).all()
    d0, _ = decode_video_ref(P, packing, 0, 0, 5, -9.0, 9.0)
    d1, n = decode_video_ref(P, packing, 0, 1, 5, -9.0, 9.0)
    assert np.array_equal(d0, d1) and n["gated_even"] == n["gated_odd"] == 0 and n["ungated_even"] > 0 and n["ungated_odd"] > 0


@pytest.mark.parametrize("packing", [1, 3])
def test_dfilter_1_with_gate_255_is_the_plain_linear_expansion(packing):
    rs = np.random.RandomState(10 + packing)
    P = rs.randint(0, 256, size=(6, 8)).astype(np.uint8)
    axis = 1 if packing == 1 else 0
    c0, c1 = _expanded_pairs(P, axis)
    v = np.moveaxis(3 * c0 + c1, 0, axis)  # the packing's weights 96 / 32 of 128, in quarter codes
    lo, hi = -20.0, 11.0
    q4 = f32((hi - lo) / (4.0 * 255))
    want = (f32(lo) + (v.astype(f32) * q4).astype(f32)).astype(f32)
    got, n = decode_video_ref(P, packing, 0, 1, 255, lo, hi)
    assert np.array_equal(got, want) and n["ungated_even"] == n["ungated_odd"] == 0


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
@pytest.mark.parametrize("packing", [1, 3])
def test_the_border_samples_clamp_inside_the_depth_region(fmt, packing):
    """whatever the gap, the image half, the spare columns, the other colour bytes or the chroma hold, disp_l is the same"""
    H, W, gap = 8, 12, 2
    for swap in (0, 1):
        setting = (packing, swap, 1)
        codes = scene_codes(H, W, packing, 0, -12.0, 12.0)
        got = []
        for seed in (1, 2):
            frame = build_video_frame(H, W, fmt, setting, gap, codes, seed=seed, extra_cols=4)
            got.append(depth_video_ref(frame, H, W, fmt, 0, setting, gap, 0, 1, 255, -12.0, 12.0, 1, 0.5))
        assert np.array_equal(got[0][1], got[1][1]) and not np.array_equal(got[0][0], got[1][0])
        want, n = decode_video_ref(codes, packing, 0, 1, 255, -12.0, 12.0)
        assert np.array_equal(got[0][1], want) and n["clamped_first"] > 0 and n["clamped_last"] > 0
        edge = want[:, 0] if packing == 1 else want[0]
        assert np.array_equal(edge, decode_ref(codes[:, 0] if packing == 1 else codes[0], "u8", -12.0, 12.0))  # n = k: 3 c0 + c0


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
@pytest.mark.parametrize("packing", [0, 1, 2, 3])
def test_swapping_the_halves_and_setting_swap_gives_the_same(fmt, packing):
    H, W, gap = 8, 12, 2
    filt = 1 if packing & 1 else 0
    Hp, Wp = packed_eye_shape(H, W, packing)
    rows_f = frame_shape(H, W, packing, gap)[0]
    a = build_video_frame(H, W, fmt, (packing, 0, filt), gap, scene_codes(H, W, packing, 1, LO, HI), seed=4)
    b = np.zeros_like(a)
    for e in (0, 1):  # half e of a, where swap 1 looks for it
        (ra, ca), (rb, cb) = eye_origin(e, H, W, packing, 0, gap), eye_origin(e, H, W, packing, 1, gap)
        b[rb:rb + Hp, cb:cb + Wp] = a[ra:ra + Hp, ca:ca + Wp]  # the pixels, or the Y samples
        if fmt == "nv12":
            b[rows_f + rb // 2:rows_f + (rb + Hp) // 2, cb:cb + Wp] = a[rows_f + ra // 2:rows_f + (ra + Hp) // 2, ca:ca + Wp]
    assert not np.array_equal(a, b)
    args = (1, 0, 0, LO, HI, 1, GATE)
    ra_ = depth_video_ref(a, H, W, fmt, 2, (packing, 0, filt), gap, *args)
    rb_ = depth_video_ref(b, H, W, fmt, 2, (packing, 1, filt), gap, *args)
    for x, y in zip(ra_[:5], rb_[:5]):
        assert np.array_equal(x, y)
    assert ra_[5] == rb_[5] and ra_[4].any()


# ----------------------------------------------------------------------------- the test scene
# (name, format, matrix, H, W, (packing, swap, filter), gap, extra columns, range, dfilter, dgate, fill, elem_sz): the cases of
# tests/test_gpu_depth_video.py.  lo, hi and the gate of step E are the scene's
LO, HI, GATE = -12.0, 12.0, 0.5
CASES = [
    ("bgr-sbs-9x37", "bgr", 0, 9, 37, (0, 0, 0), 3, 5, 0, 0, 0, 1, 3),
    ("bgr-tab-9x37", "bgr", 0, 9, 37, (2, 1, 0), 3, 0, 0, 0, 0, 0, 3),
    ("bgr-half-sbs-10x38", "bgr", 0, 10, 38, (1, 0, 0), 0, 0, 1, 1, 2, 1, 3),
    ("bgr-half-tab-10x37", "bgr", 0, 10, 37, (3, 1, 1), 0, 0, 0, 1, 3, 0, 3),
    ("bgr4-half-sbs-10x38", "bgr", 0, 10, 38, (1, 1, 1), 1, 2, 1, 0, 0, 1, 4),
    ("nv12-sbs-6x44", "nv12", 0, 6, 44, (0, 1, 0), 2, 0, 1, 0, 0, 0, 3),
    ("nv12-half-sbs-8x36", "nv12", 1, 8, 36, (1, 0, 1), 0, 0, 1, 1, 2, 1, 3),
    ("nv12-half-tab-12x300", "nv12", 2, 12, 300, (3, 0, 0), 0, 0, 0, 1, 3, 1, 3),
]
CASE = {c[0]: c for c in CASES}


def case_frame(name, k=0):
    """frame k of a case, read-only"""
    _, fmt, _, H, W, setting, gap, extra, rng, _, _, _, elem_sz = CASE[name]
    frame = build_video_frame(H, W, fmt, setting, gap, scene_codes(H, W, setting[0], rng, LO, HI, k), seed=k + 1, extra_cols=extra, elem_sz=elem_sz)
    frame.setflags(write=False)
    return frame


def case_ref(name, k=0):
    _, fmt, matrix, H, W, setting, gap, _, rng, dfilter, dgate, fill, _ = CASE[name]
    return depth_video_ref(case_frame(name, k), H, W, fmt, matrix, setting, gap, rng, dfilter, dgate, LO, HI, fill, GATE)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_the_scene_meets_every_case(name):
    """the conditions tests/test_gpu_depth_video.py relies on, as conditions on the inputs: every case of steps B to E, and of a
    squeezed depth picture every kind of pair at both parities and both clamps; with range 1 samples outside 16 .. 235"""
    _, fmt, matrix, H, W, setting, gap, _, rng, dfilter, dgate, fill, _ = CASE[name]
    n = case_ref(name)[5]
    need = [c for c in COUNTS if not (c == "mirrors_rejected" and W > 64)]
    if setting[0] & 1:
        need += ["clamped_first", "clamped_last"]
        if dfilter:
            need += ["gated_even", "gated_odd", "ungated_even", "ungated_odd"]
    if rng:
        need += ["below_16", "above_235"]
    assert all(n[c] > 0 for c in need), (name, n)


def test_the_cases_cover_every_setting():
    assert {c[1] for c in CASES} == {"bgr", "nv12"} and {c[5][0] for c in CASES if c[1] == "bgr"} == {0, 1, 2, 3}
    assert {c[5][0] for c in CASES if c[1] == "nv12"} | {2} == {0, 1, 2, 3}  # NV12 with packing 2: the widest row of the GPU tests
    assert {c[2] for c in CASES if c[1] == "nv12"} | {3} == {0, 1, 2, 3}     # ... which runs matrix 3
    for idx, both in ((8, {0, 1}), (9, {0, 1}), (11, {0, 1})):               # range, dfilter, fill
        assert {c[idx] for c in CASES} == both
    assert {c[5][1] for c in CASES} == {0, 1} and {c[5][2] for c in CASES if c[5][0] & 1} == {0, 1} and 4 in {c[12] for c in CASES}


# ----------------------------------------------------------------------------- the two tools
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_take_depth_video_option():
    from stm_amd import video
    argv = ["x", "--depth-video", "1", "1", "4", "12", "-3.5", "--cut"]
    assert video.take_depth_video_option(argv) == (1, 1, 4, 12.0, -3.5, 0, 0.0) and argv == ["x", "--cut"]
    argv = ["--depth-video", "0", "0", "0", "0", "16", "1", "0.5", "y"]
    assert video.take_depth_video_option(argv) == (0, 0, 0, 0.0, 16.0, 1, 0.5) and argv == ["y"]
    assert video.take_depth_video_option(["x"]) is None
    for bad in (["--depth-video"], ["--depth-video", "0", "0", "0", "1"], ["--depth-video", "2", "0", "0", "0", "16"],
                ["--depth-video", "0", "2", "0", "0", "16"], ["--depth-video", "0", "1", "256", "0", "16"], ["--depth-video", "0", "1", "-1", "0", "16"],
                ["--depth-video", "0", "0", "0", "1", "1"], ["--depth-video", "0", "0", "0", "nan", "1"], ["--depth-video", "0", "0", "0", "0", "5000"],
                ["--depth-video", "0", "0", "0", "0", "16", "1"], ["--depth-video", "0", "0", "0", "0", "16", "2", "0.5"],
                ["--depth-video", "0", "0", "0", "0", "16", "1", "-1"], ["--depth-video", "0.5", "0", "0", "0", "16"],
                ["--depth-video", "0", "0", "x", "0", "16"]):
        with pytest.raises((ValueError, IndexError)):
            video.take_depth_video_option(list(bad))


def test_the_tools_refuse_a_malformed_depth_video_option(tmp_path, capsys):
    plane = str(tmp_path / "stack.npy")
    np.save(plane, np.zeros((2, 4, 6), np.uint8))
    np.save(str(tmp_path / "one.npy"), np.zeros((4, 6), np.uint8))
    ok = ["--depth-video", "0", "0", "0", "0", "16"]
    vid, img = _tool("stm_video"), _tool("stm_image")
    for tail in (["--depth-video"], ["--depth-video", "0", "0", "0", "3", "3"], ["--depth-video", "3", "0", "0", "0", "16"], ok + ["1"],
                 ["--depth-video", "0", "1", "4", "0", "16"],  # dfilter 1 on a full-size depth picture
                 ["--depth-video", "0", "1", "4", "0", "16", "--packing", "2", "0", "0", "0"], ok + ["--align", "0", "0", "0"],
                 ok + ["--match", "4", "6", "0.5"], ["--subpixel"] + ok, ["--temporal"] + ok, ok + ["--depth-input", plane, "0", "16"]):
        assert vid.main(["stm_video"] + ["x"] * 16 + tail) == -1, tail
        assert "--depth-video RANGE DFILTER DGATE LO HI" in capsys.readouterr().out
    for tail in (["--depth-video"], ["--depth-video", "0", "0", "0", "3", "3"], ["--depth-video", "0", "0", "300", "0", "16"], ok + ["7", "1"],
                 ["--depth-video", "0", "1", "4", "0", "16"], ["--packing", "1", "0", "0", "0"], ok + ["--packing", "1", "0", "0"],
                 ok + ["--align", "0", "0", "0"], ["--interp"] + ok, ok + ["--depth-input", str(tmp_path / "one.npy"), "0", "16"]):
        assert img.main(["stm_image"] + ["x"] * 17 + tail) == -1, tail
        assert "--depth-video RANGE DFILTER DGATE LO HI" in capsys.readouterr().out
