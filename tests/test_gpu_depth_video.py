"""Packed 2D-plus-depth video frames as a frame stream's input on the GPU (stm_stream_input_packed_depth).
Everything bit for bit, seven frames per stream (both slots run eager, capture their graph and replay it):
  (a) the eye: disp_l, disp_r and -- through a two-view quilt whose tiles are the right and the left image verbatim -- img_l and img_r
      against test_depth_video_ref's depth_video_ref;
  (b) packings 0 and 2 with range 0: the three outputs equal those of an stm_stream_input_depth u8 stream fed the reference-unpacked
      image and the cut-out sample plane;
  (c) every other case: the three outputs equal those of an stm_stream_input_depth f32 stream fed the reference-unpacked image and the
      reference-decoded plane, its clamp limits one unit beyond the plane's range -- under stages 3 and 3 | 0x800, lens mode 3, a
      quilt with NV12 output, the overlay, u8 maps, and the cut detector with the automatic active area, one setting a case;
  (d) every refusal, in both directions, leaves the stream as it was;
  (e) a stream without the call equals a fresh-process stream.
The cases are test_depth_video_ref.CASES (BGR 9 x 37 side by side with a gap and spare columns, 9 x 37 top and bottom, 10 x 38 half
width, 10 x 37 half height, 4-byte pixels; NV12 6 x 44, 8 x 36 half width, 12 x 300 half height) and NV12 2 x 8192 top and bottom, the
row whose keys need the LDS opt-in.  The references of a case are computed once and shared."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_depth_video_ref import CASE, CASES, GATE, HI, LO, build_video_frame, case_frame, depth_video_ref, split_frame
from test_lens_ref import LINEAR_WARP
from test_overlay_ref import ANGLE, PANEL, random_overlay
from test_packing_ref import eye_origin, frame_shape, packed_eye_shape
from test_quilt_ref import quilt_ref

pytestmark = pytest.mark.gpu

N = 7
f32 = np.float32
f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def _params(num_views=8):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=16, zero_disp=8, usd=17, lsd=8, num_views=num_views, angle=ANGLE)


def setting_of(name):
    """FrameStream's depth_video tuple of a case, and its row length"""
    _, fmt, matrix, H, W, (packing, swap, filt), gap, extra, rng, dfilter, dgate, fill, _ = CASE[name]
    return (fmt, matrix, packing, swap, filt, gap, rng, dfilter, dgate, LO, HI, fill, GATE), frame_shape(H, W, packing, gap)[1] + extra


@functools.lru_cache(maxsize=None)
def frames_of(name):
    return tuple(case_frame(name, k) for k in range(N))


@functools.lru_cache(maxsize=None)
def reference(name):
    """[(img_l, disp_l, img_r, disp_r, holes, counts)] of the N frames, read-only"""
    _, fmt, matrix, H, W, setting, gap, _, rng, dfilter, dgate, fill, _ = CASE[name]
    out = []
    for frame in frames_of(name):
        r = depth_video_ref(frame, H, W, fmt, matrix, setting, gap, rng, dfilter, dgate, LO, HI, fill, GATE)
        for a in r[:5]:
            a.setflags(write=False)
        out.append(r)
    return tuple(out)


def drive(fs, frames, submit, collect=None):
    """the frames through a stream, two in flight; returns [(disp_l, disp_r, frame) + collect(fs)] as copies, and closes the stream"""
    try:
        got, pending = [], 0

        def take():
            r = fs.collect()
            assert r is not None and r[0] == len(got)
            extra = () if collect is None else (collect(fs),)
            got.append(tuple(None if a is None else np.array(a) for a in r[1:]) + extra)
        for f in frames:
            if pending == 2:
                take()
                pending -= 1
            assert submit(fs, f) >= 0
            pending += 1
        while pending:
            take()
            pending -= 1
    finally:
        fs.close()
    return got


def run_video(name, frames=None, collect=None, **kw):
    from stm_amd import video
    H, W = CASE[name][3:5]
    dv, pitch = setting_of(name)
    fs = video.FrameStream(H, W, kw.pop("params", None) or _params(), depth_video=dv, depth_pitch=pitch, **kw)
    assert fs.in_shape == frames_of(name)[0].shape
    return drive(fs, frames_of(name) if frames is None else frames, lambda s, f: s.submit(f), collect)


def run_depth(H, W, fmt, lo, hi, fill, pairs, collect=None, **kw):
    """the existing image-plus-depth stream on (image, plane) pairs"""
    from stm_amd import video
    fs = video.FrameStream(H, W, kw.pop("params", None) or _params(), depth_input=(fmt, lo, hi, fill, GATE), **kw)
    return drive(fs, pairs, lambda s, p: s.submit_depth(*p), collect)


def same_outputs(got, want, what):
    assert len(got) == len(want) == N
    for k, (g, w) in enumerate(zip(got, want)):
        for i, part in enumerate(("disp_l", "disp_r", "frame")):
            assert (g[i] is None and w[i] is None) or (g[i].dtype == w[i].dtype and np.array_equal(g[i], w[i])), (what, k, part)
        assert g[3:] == w[3:], (what, k, g[3:], w[3:])


def decoded_pairs(name):
    """(c)'s input: the reference-unpacked image and the reference-decoded plane of every frame, and limits one unit beyond its range"""
    ref = reference(name)
    lo = float(min(r[1].min() for r in ref)) - 1.0
    hi = float(max(r[1].max() for r in ref)) + 1.0
    return [(r[0], r[1]) for r in ref], lo, hi


def against_f32_stream(name, **kw):
    H, W, fill = CASE[name][3], CASE[name][4], CASE[name][11]
    pairs, lo, hi = decoded_pairs(name)
    collect = kw.pop("collect", None)
    got = run_video(name, collect=collect, **dict(kw))
    want = run_depth(H, W, "f32", lo, hi, fill, pairs, collect=collect, **dict(kw))
    same_outputs(got, want, name)
    return got


# ----------------------------------------------------------------------------- (a) the eye
@pytest.mark.parametrize("name", [c[0] for c in CASES if c[12] == 3])
def test_the_eye(gpu_ready, name):
    H, W = CASE[name][3:5]
    ref = reference(name)
    got = run_video(name, params=_params(2), out_rows=H, out_cols=2 * W, layout=(1, 2, 1, 0, 0))
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[0].dtype == np.float32 and np.array_equal(g[0], r[1]), (k, "disp_l", int((g[0] != r[1]).sum()))
        assert np.array_equal(g[1], r[3]), (k, "disp_r", int((g[1] != r[3]).sum()))
        want = quilt_ref([r[2], r[0]], 2, 1, 0, 0, H, 2 * W)
        assert np.array_equal(g[2][:, W:], want[:, W:]), (k, "img_l", int((g[2][:, W:] != want[:, W:]).sum()))
        assert np.array_equal(g[2], want), (k, "img_r", int((g[2] != want).sum()))
    assert any(not np.array_equal(a[3], b[3]) for a, b in zip(ref, ref[1:]))  # the box moves: the replayed graphs see new data


def _c_stream(lib, H, Wsbs, W, Ho, Wo, E, views):
    p = _params(views)
    return lib.stm_stream_create(H, Wsbs, W, Ho, Wo, E, views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd,
                                 p.lsd, p.thresh_s, p.thresh_h)


def _c_frames(lib, h, flats, H, W, out_shape):
    got = []
    for k, flat in enumerate(flats):
        flat = np.ascontiguousarray(flat).reshape(-1)
        assert lib.stm_stream_submit(h, flat.ctypes.data_as(u8p)) == k
        dl, dr, out = np.empty((H, W), f32), np.empty((H, W), f32), np.empty(out_shape, np.uint8)
        assert lib.stm_stream_collect(h, dl.ctypes.data_as(f32p), dr.ctypes.data_as(f32p), out.ctypes.data_as(u8p)) == k
        got.append((dl, dr, out))
    return got


def test_the_eye_and_the_frame_with_4_byte_pixels(gpu_ready, stm):
    """elem_sz 4 through the C calls: the maps, the two images through the quilt's area filter on tiles of the views' own size, and the
    default frame against the f32 depth stream's on 4-byte images"""
    lib = stm.lib()
    name = "bgr4-half-sbs-10x38"
    H, W = CASE[name][3:5]
    dv, pitch = setting_of(name)
    ref = reference(name)
    args = (0,) + dv[1:]
    h = _c_stream(lib, H, pitch, W, H, 2 * W, 4, 2)
    try:
        assert lib.stm_stream_set_layout(h, 1, 2, 1, 0, 1) == 0 and lib.stm_stream_input_packed_depth(h, *args) == 0
        got = _c_frames(lib, h, frames_of(name), H, W, (H, 2 * W, 4))
    finally:
        lib.stm_stream_destroy(h)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g[0], r[1]) and np.array_equal(g[1], r[3]), k
        want = quilt_ref([r[2], r[0]], 2, 1, 0, 1, H, 2 * W)
        assert np.array_equal(g[2][..., :3], want), (k, int((g[2][..., :3] != want).sum()))
    pairs, lo, hi = decoded_pairs(name)
    off = (H * W * 4 + 15) // 16 * 16
    flats = []
    for img, plane in pairs:
        flat = np.zeros(off + plane.nbytes, np.uint8)
        flat[:H * W * 4].reshape(H, W, 4)[..., :3] = img
        flat[off:] = np.ascontiguousarray(plane).view(np.uint8).reshape(-1)
        flats.append(flat)
    outs = []
    for video_stream in (True, False):
        h = _c_stream(lib, H, pitch if video_stream else W, W, H, W, 4, 8)
        try:
            if video_stream:
                assert lib.stm_stream_input_packed_depth(h, *args) == 0
            else:
                assert lib.stm_stream_input_depth(h, 0, lo, hi, dv[11], GATE) == 0
            outs.append(_c_frames(lib, h, frames_of(name) if video_stream else flats, H, W, (H, W, 4)))
        finally:
            lib.stm_stream_destroy(h)
    for k, (g, w) in enumerate(zip(*outs)):
        assert all(np.array_equal(a, b) for a, b in zip(g, w)), k


def test_the_widest_row(gpu_ready):
    """NV12 2 x 8192, top and bottom, matrix 3: the keys take 64 KiB + 64 bytes of LDS and the launch opts in.  Seven frames that
    differ in the image and in the depth picture, two in flight: both slots run eager, capture and replay on new data"""
    from stm_amd import video
    H, W = 2, 8192
    frames, refs = [], []
    for k in range(N):
        codes = np.random.RandomState(3 + k).randint(0, 256, size=(H, W)).astype(np.uint8)
        codes[:, 4000 + 100 * k:4200 + 100 * k] = 255
        frames.append(build_video_frame(H, W, "nv12", (2, 0, 0), 0, codes, seed=9 + k))
        refs.append(depth_video_ref(frames[-1], H, W, "nv12", 3, (2, 0, 0), 0, 0, 0, 0, -20.0, 20.0, 1, GATE))
    fs = video.FrameStream(H, W, _params(2), H, 2 * W, layout=(1, 2, 1, 0, 0), depth_video=("nv12", 3, 2, 0, 0, 0, 0, 0, 0, -20.0, 20.0, 1, GATE))
    assert fs.in_shape == (6, W)
    got = drive(fs, frames, lambda s, f: s.submit(f))
    for k, (g, (img, dl, img_r, dr, holes, _)) in enumerate(zip(got, refs)):
        assert np.array_equal(g[0], dl) and np.array_equal(g[1], dr), k
        assert np.array_equal(g[2][:, :W], img_r) and np.array_equal(g[2][:, W:], img), k
        assert holes.any()
    assert not np.array_equal(refs[0][3], refs[1][3])


# ----------------------------------------------------------------------------- (b) the u8 depth stream on the cut-out plane
@pytest.mark.parametrize("name", [c[0] for c in CASES if not c[5][0] & 1 and c[8] == 0])
def test_full_packings_equal_the_u8_depth_stream(gpu_ready, name):
    _, fmt, _, H, W, (packing, swap, _), gap, _, _, _, _, fill, _ = CASE[name]
    Hp, Wp = packed_eye_shape(H, W, packing)
    r0, c0 = eye_origin(1, H, W, packing, swap, gap)
    pairs = [(r[0], np.ascontiguousarray(split_frame(f, fmt)[1][r0:r0 + Hp, c0:c0 + Wp])) for f, r in zip(frames_of(name), reference(name))]
    same_outputs(run_video(name), run_depth(H, W, "u8", LO, HI, fill, pairs), name)


# ----------------------------------------------------------------------------- (c) the f32 depth stream on the decoded plane
@pytest.mark.parametrize("stages", [3, 3 | LINEAR_WARP], ids=["0x3", "0x803"])
def test_half_width_bgr_under_both_stage_words(gpu_ready, stages):
    against_f32_stream("bgr-half-sbs-10x38", stages=stages)


def test_half_height_bgr_under_lens_mode_3(gpu_ready):
    against_f32_stream("bgr-half-tab-10x37", stages=3 | LINEAR_WARP, lens=(3,) + PANEL)


def test_nv12_side_by_side_under_a_quilt_with_nv12_output(gpu_ready):
    got = against_f32_stream("nv12-sbs-6x44", out_rows=44, out_cols=176, layout=(1, 4, 2, 1, 1), output=(1, 1))  # even tiles
    assert got[0][2].shape == (66, 176)


def test_half_width_nv12_under_the_overlay(gpu_ready):
    from stm_amd import video
    name = "nv12-half-sbs-8x36"
    H, W, fill = CASE[name][3], CASE[name][4], CASE[name][11]
    base = run_video(name)
    pairs, lo, hi = decoded_pairs(name)
    ov = random_overlay(11, 3, 9)
    dv, pitch = setting_of(name)
    streams = [video.FrameStream(H, W, _params(), depth_video=dv, depth_pitch=pitch, overlay=(3, 9)),
               video.FrameStream(H, W, _params(), depth_input=("f32", lo, hi, fill, GATE), overlay=(3, 9))]
    try:
        for fs in streams:
            fs.overlay(ov, 12, 2, -2.5)
        for k, (frame, pair) in enumerate(zip(frames_of(name), pairs)):
            assert streams[0].submit(frame) == k and streams[1].submit_depth(*pair) == k
            g, w = streams[0].collect(), streams[1].collect()
            assert all(np.array_equal(a, b) for a, b in zip(g[1:], w[1:])), k
            assert not np.array_equal(g[3], base[k][2]) and np.array_equal(g[1], base[k][0]), k
    finally:
        for fs in streams:
            fs.close()


def test_half_height_nv12_with_u8_maps(gpu_ready):
    got = against_f32_stream("nv12-half-tab-12x300", maps=("u8", "both", 10.0, -10.0))
    assert got[0][0].dtype == np.uint8 and got[0][1].dtype == np.uint8


def test_cut_and_automatic_active_area_see_the_image_half_only(gpu_ready):
    """BGR 16 x 64, half width, the depth picture first.  The image has black bars of three and two rows and turns into another picture
    at frame 4; the depth picture has no bars (it is bright in those rows) and turns over at frame 2.  stm_stream_cut and
    stm_stream_active, and the outputs, equal those of the f32 depth stream fed the unpacked image: a detector that read the depth half,
    or the whole frame, would see no bars and a cut at frame 2"""
    H, W, setting, gap = 16, 64, (1, 1, 0), 0
    rs = np.random.RandomState(16)
    frames, pairs = [], []
    for k in range(N):
        image = np.random.RandomState(5).randint(0, 256, size=(H, W // 2, 3)).astype(np.uint8)
        if k >= 4:  # the same picture at a quarter of the contrast: every cell's histogram moves
            image = (image >> 2) + 100
        image[:3] = 0
        image[H - 2:] = 0
        codes = rs.randint(150, 256, size=(H, W // 2)).astype(np.uint8)
        codes[:, W // 8 + k:W // 8 + k + 6] = 20
        if k >= 2:
            codes = (255 - codes).astype(np.uint8)
            codes[:3], codes[H - 2:] = 250, 240
        frame = build_video_frame(H, W, "bgr", setting, gap, codes, seed=k, image=image)
        frame[..., 0], frame[..., 2] = frame[..., 1], frame[..., 1]  # the depth half is a grey picture; the image half keeps its G
        i0, j0 = eye_origin(0, H, W, 1, 1, gap)
        frame[i0:i0 + H, j0:j0 + W // 2] = image
        frames.append(frame)
        r = depth_video_ref(frame, H, W, "bgr", 0, setting, gap, 0, 1, 6, LO, HI, 0, GATE)
        pairs.append((r[0], r[1]))
    from stm_amd import video
    kw = dict(cut=True, active_auto=(24, 10, 300, 2), active_fill=0.0)
    collect = lambda fs: (fs.cut(), fs.active())  # noqa: E731
    fs = video.FrameStream(H, W, _params(), depth_video=("bgr", 0, 1, 1, 0, gap, 0, 1, 6, LO, HI, 0, GATE), **kw)
    got = drive(fs, frames, lambda s, f: s.submit(f), collect)
    lo, hi = float(min(p[1].min() for p in pairs)) - 1.0, float(max(p[1].max() for p in pairs)) + 1.0
    want = run_depth(H, W, "f32", lo, hi, 0, pairs, collect=collect, **kw)
    same_outputs(got, want, "cut")
    assert [g[3][0][0] for g in got] == [1, 0, 0, 0, 1, 0, 0]
    assert got[-1][3][1][:4] != (0, H, 0, W)  # the bars were found


# ----------------------------------------------------------------------------- (d) the refusals, in both directions
def test_refusals_leave_the_stream_as_it_was(gpu_ready, stm):
    from stm_amd import video
    lib = stm.lib()
    name = "bgr-half-sbs-10x38"
    H, W = CASE[name][3:5]
    dv, pitch = setting_of(name)
    ok = (0,) + dv[1:]
    ref = reference(name)
    nan, inf = float("nan"), float("inf")
    lib.stm_set_error_mode(1)
    streams = []

    def stream(h=H, w=W, **kw):
        streams.append(video.FrameStream(h, w, _params(), **kw))
        return streams[-1]

    def refused(call, *words):
        lib.stm_d_filter_median(None, 0, 0)  # plant a known message
        assert call() == -1
        err = lib.stm_last_error()
        assert all(wd in err for wd in words), err

    def but(**change):
        names = ["format", "matrix", "packing", "swap", "filter", "gap", "range", "dfilter", "dgate", "lo", "hi", "fill", "gate"]
        a = list(ok)
        for key, v in change.items():
            a[names.index(key)] = v
        return tuple(a)
    from stm_amd import rectify
    rec36 = np.ascontiguousarray(np.stack([rectify.identity(), rectify.identity()]), dtype=f32)
    try:
        fs = stream(depth_video=dv, depth_pitch=pitch)
        sv = lib.stm_stream_input_packed_depth
        me = b"stream_input_packed_depth:"
        for bad in (2, -2, 7):
            refused(lambda: sv(fs._h, *but(format=bad)), me, b"format")
        for key, bads in (("packing", (-1, 4)), ("swap", (-1, 2)), ("filter", (-1, 2)), ("gap", (-1,)), ("range", (-1, 2)), ("dfilter", (-1, 2)),
                          ("dgate", (-1, 256)), ("fill", (-1, 2))):
            for bad in bads:
                refused(lambda: sv(fs._h, *but(**{key: bad})), me, key.encode())
        refused(lambda: sv(fs._h, *but(packing=0, filter=0, dfilter=1)), me, b"dfilter")  # a full-size depth picture is not expanded
        refused(lambda: sv(fs._h, *but(packing=2, filter=0, dfilter=1)), me, b"dfilter")
        refused(lambda: sv(fs._h, *but(packing=0, filter=1, dfilter=0)), me, b"filter")   # stm_demux_packed's own rule
        refused(lambda: sv(fs._h, *but(gap=5)), me, b"num_cols_sbs")                      # ... and its geometry
        refused(lambda: sv(fs._h, *but(format=1, matrix=4)), me)                          # stm_demux_nv12_packed's rules: 38 is no multiple of 4
        for a, b in ((3.0, 3.0), (3.0, 3.0 + 1.0 / 128.0), (nan, 1.0), (1.0, nan), (inf, 0.0), (0.0, -inf), (5000.0, 0.0), (0.0, -5000.0)):
            refused(lambda: sv(fs._h, *but(lo=a, hi=b)), me, b"lo", b"hi")
        for g in (nan, inf, -0.5, 5000.0):
            refused(lambda: sv(fs._h, *but(fill=1, gate=g)), me, b"gate")
        assert sv(fs._h, *but(fill=0, gate=nan)) == 0  # fill 0 does not look at the gate
        assert sv(fs._h, *ok) == 0                     # ... and back to the test's setting
        # the other direction: each names its own entry and this input
        other = [("stream_input_depth:", lambda: lib.stm_stream_input_depth(fs._h, 2, LO, HI, 0, 0.0)),
                 ("stream_set_input:", lambda: lib.stm_stream_set_input(fs._h, 1, 0)),
                 ("stream_set_input:", lambda: lib.stm_stream_set_input(fs._h, 0, 0)),
                 ("stream_set_packing:", lambda: lib.stm_stream_set_packing(fs._h, 1, 0, 0, 0)),
                 ("stream_set_match_size:", lambda: lib.stm_stream_set_match_size(fs._h, 5, 19, 0.5)),
                 ("stream_set_align:", lambda: lib.stm_stream_set_align(fs._h, 1, 0.5, 0.0, 0.0)),
                 ("stream_set_balance:", lambda: lib.stm_stream_set_balance(fs._h, 2, None)),
                 ("stream_rectify:", lambda: lib.stm_stream_rectify(fs._h, 1, rec36.ctypes.data_as(f32p), 0)),
                 ("stream_set_stages:", lambda: lib.stm_stream_set_stages(fs._h, 3 | 0x200)),
                 ("stream_set_stages:", lambda: lib.stm_stream_set_stages(fs._h, 3 | 0x2000))]
        for who, call in other:
            refused(call, who.encode(), b"packed depth video input", b"stm_stream_input_packed_depth")
        assert lib.stm_stream_set_stages(fs._h, 3 | 0x800) == 0 and lib.stm_stream_set_stages(fs._h, 3) == 0
        assert lib.stm_stream_input_depth(fs._h, -1, 0.0, 0.0, 0, 0.0) == 0  # off is what the other input already is
        # after all of that the stream still produces frame 0, and refuses the call after it
        assert fs.in_shape == frames_of(name)[0].shape and fs.submit(frames_of(name)[0]) == 0
        refused(lambda: sv(fs._h, *ok), me, b"first submit")
        refused(lambda: sv(fs._h, *but(format=-1)), me, b"first submit")
        refused(lambda: sv(fs._h, *but(format=7)), me, b"format")  # the broken argument wins
        k, dl, dr, out = fs.collect()
        assert k == 0 and np.array_equal(dl, ref[0][1]) and np.array_equal(dr, ref[0][3])
        assert np.array_equal(out, run_video(name)[0][2])
        # a stream that already has what such a frame does not go with
        for kw, word in ((dict(depth_input=("u8", LO, HI), depth_pitch=2 * W), b"depth input"), (dict(h=12, w=40, input_format="nv12"), b"NV12"),
                         (dict(packing=(0, 1, 0, 0)), b"packing"), (dict(match=(5, 19, 0.5)), b"match size"), (dict(align=(0.5, 0.0, 0.0)), b"alignment"),
                         (dict(balance=np.tile(np.arange(256, dtype=np.uint8)[::-1], (3, 1))), b"balance"),
                         (dict(stages=3 | 0x400), b"stages"), (dict(stages=3 | 0x2000), b"stages")):
            s = stream(**kw)
            refused(lambda: sv(s._h, *but(packing=0, filter=0, dfilter=0, gap=0)), me, word)
            assert sv(s._h, *but(format=-1)) == 0  # off is what such a stream already is
        s = stream(rectify=(rectify.identity(), rectify.identity()))
        refused(lambda: sv(s._h, *but(packing=0, filter=0, dfilter=0, gap=0)), me, b"rectification")
        wide = stream(2, 8200)
        refused(lambda: sv(wide._h, *but(packing=0, filter=0, dfilter=0, gap=0)), me, b"num_cols", b"8192")
        with pytest.raises(ValueError, match="stm_stream_input_packed_depth"):
            video.FrameStream(H, W, _params(), depth_video=("bgr", 0, 1, 0, 0, 0, 0, 0, 0, 2.0, 2.0))
        # switched on and off again: a stereo stream as it was
        s = stream()
        assert sv(s._h, *but(packing=0, filter=0, dfilter=0, gap=0)) == 0 and sv(s._h, *but(format=-1)) == 0
        assert lib.stm_stream_set_stages(s._h, 3 | 0x200) == 0
    finally:
        lib.stm_set_error_mode(0)
        for s in streams:
            s.close()


# ----------------------------------------------------------------------------- (e) a stream without the call
def _stereo_digest(switch=False):
    """sha256 over the maps and frames of a plain stereo stream; switch: the packed depth input switched on and off again first"""
    from stm_amd import video
    import test_gpu_stream_maps as t
    H, W = t.SHAPES["24x40"][:2]
    fs = video.FrameStream(H, W, t._params("24x40"))
    h = hashlib.sha256()
    try:
        if switch:
            fs.set_depth_video("nv12", 1, 1, 1, 1, 0, 1, 1, 4, -3.0, 9.0, 1, 0.25)
            assert fs.in_shape == (36, 2 * W)
            fs.set_depth_video("off")
            assert fs.in_shape == (H, 2 * W, 3)
        for k, f in enumerate(t.frames_of("24x40")):
            assert fs.submit(f) == k
            for a in fs.collect()[1:]:
                h.update(np.ascontiguousarray(a).tobytes())
    finally:
        fs.close()
    return h.hexdigest()


def test_a_stream_without_the_call_is_a_fresh_process_stream(gpu_ready):
    """after packed depth streams have run in this process, a stereo stream -- untouched, or with the input switched on and off again --
    gives the bytes of a stereo stream in a process that never heard of the setting"""
    run_video("nv12-half-sbs-8x36")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_depth_video as t\n"
            "print('digest', t._stereo_digest())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "digest " in r.stdout, r.stdout + r.stderr
    fresh = r.stdout.strip().split("digest ")[-1]
    assert _stereo_digest() == fresh and _stereo_digest(switch=True) == fresh
