"""Image-plus-depth input of a frame stream on the GPU (stm_stream_input_depth): the decoded plane, the
synthesised right map and right image bit for bit against test_depth_input_ref's decode_ref and eye_ref, the frame against the
renderer's numpy statements on (img, img_r, disp_l, disp_r), the stream's settings on this input, the refusals in both directions.
Seven frames per stream: both slots run eager, capture their graph and replay it.  Shapes: 9 x 37 (a row shorter than a wave), 16 x
64, 21 x 83 (odd W: unaligned plane rows, and the plane does not start where the image ends), 5 x 300 (more than one column per lane
in the scans), one case with 4-byte pixels and one with an image pitch of 2 W.  The reference of a configuration is computed once
and shared."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_depth_input_ref import COUNTS, PLANE_DTYPE, decode_ref, eye_ref, scene_disp, scene_image, scene_plane
from test_depth_ref import depth_fit_ref
from test_lens_ref import LINEAR_WARP, chain_views, render_chain, render_lens_ref
from test_overlay_ref import ANGLE, PANEL, overlay_ref, random_overlay, subpixel_shift_ref
from test_quilt_ref import quilt_ref, render_quilt_ref
from test_stream_maps_ref import plane_ref
from test_temporal_ref import SEQ, mixed_sequence

pytestmark = pytest.mark.gpu

N = 7
GATE = 0.5
SHAPES = {"9x37": (9, 37), "16x64": (16, 64), "21x83": (21, 83), "5x300": (5, 300)}
LIMITS = {"f32": (-8.0, 7.0), "u8": (12.0, -12.0), "u16": (-12.0, 12.0)}  # f32: both clamps fire on the scene; u8: lo > hi
f32 = np.float32
f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def _params(num_views=8):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=16, zero_disp=8, usd=17, lsd=8, num_views=num_views, angle=ANGLE)


@functools.lru_cache(maxsize=None)
def inputs(shape, fmt, pitch=None, elem_sz=3):
    """the N frames of a configuration: [(image, plane)], read-only"""
    H, W = SHAPES[shape]
    lo, hi = LIMITS[fmt]
    img = scene_image(H, W, pitch, elem_sz)
    img.setflags(write=False)
    out = []
    for k in range(N):
        plane = np.ascontiguousarray(scene_plane(H, W, fmt, lo, hi, k), dtype=PLANE_DTYPE[fmt])
        plane.setflags(write=False)
        out.append((img, plane))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(shape, fmt, fill, pitch=None, elem_sz=3):
    """[(disp_l, img_r, disp_r, holes, counts)] of the N frames, read-only"""
    lo, hi = LIMITS[fmt]
    out = []
    for img, plane in inputs(shape, fmt, pitch, elem_sz):
        dl = decode_ref(plane, fmt, lo, hi)
        img_r, dr, holes, n = eye_ref(img, dl, fill, GATE)
        for a in (dl, img_r, dr, holes):
            a.setflags(write=False)
        out.append((dl, img_r, dr, holes, n))
    return tuple(out)


def run_depth(shape, fmt, fill, frames=None, collect=None, pitch=None, **kw):
    """the frames through a FrameStream with depth input, two in flight; returns [(disp_l, disp_r, frame) + collect(fs)] as copies"""
    from stm_amd import video
    H, W = SHAPES[shape] if isinstance(shape, str) else shape
    lo, hi = kw.pop("limits", None) or LIMITS[fmt]
    fs = video.FrameStream(H, W, kw.pop("params", None) or _params(), depth_input=(fmt, lo, hi, fill, GATE), depth_pitch=pitch, **kw)
    try:
        got, pending = [], 0

        def take():
            r = fs.collect()
            assert r is not None and r[0] == len(got)
            extra = () if collect is None else (collect(fs),)
            got.append(tuple(None if a is None else np.array(a) for a in r[1:]) + extra)
        for img, plane in (inputs(shape, fmt, pitch) if frames is None else frames):
            if pending == 2:
                take()
                pending -= 1
            assert fs.submit_depth(img, plane) >= 0
            pending += 1
        while pending:
            take()
            pending -= 1
    finally:
        fs.close()
    return got


def check_maps(got, ref):
    assert len(got) == len(ref) == N
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[0].dtype == np.float32 and np.array_equal(g[0], r[0]), (k, "disp_l", int((g[0] != r[0]).sum()))
        assert np.array_equal(g[1], r[2]), (k, "disp_r", int((g[1] != r[2]).sum()))


def chain_of(orc, img, r):
    return render_chain(orc, np.ascontiguousarray(img[:, :r[0].shape[1], :3]), r[1], r[0], r[2])


# ----------------------------------------------------------------------------- 1. the eye
@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("fmt", ["f32", "u8", "u16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_eye(gpu_ready, shape, fmt, fill):
    """disp_l, disp_r and -- through a two-view quilt whose tiles are the right and the left image verbatim -- img_r"""
    H, W = SHAPES[shape]
    ref = reference(shape, fmt, fill)
    for r in ref:  # conditions on the inputs: every case of steps B to E occurs in every frame
        assert all(r[4][c] > 0 for c in COUNTS if not (c == "mirrors_rejected" and W > 64)), r[4]
    order = 0 if fill == 0 else 2
    got = run_depth(shape, fmt, fill, params=_params(2), out_rows=H, out_cols=2 * W, layout=(1, 2, 1, order, 0))
    check_maps(got, ref)
    for k, (g, r, (img, _)) in enumerate(zip(got, ref, inputs(shape, fmt))):
        want = quilt_ref([r[1], img], 2, 1, order, 0, H, 2 * W)
        assert np.array_equal(g[2], want), (k, "img_r", int((g[2] != want).sum()))
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(ref, ref[1:]))  # the box moves: the replayed graphs see new data


def test_the_eye_from_an_image_with_a_pitch(gpu_ready):
    """num_cols_sbs = 2 W: the renderer reads the kernel's tight copy of the image"""
    shape, fmt, fill = "21x83", "u8", 1
    H, W = SHAPES[shape]
    ref = reference(shape, fmt, fill, pitch=2 * W)
    got = run_depth(shape, fmt, fill, pitch=2 * W, params=_params(2), out_rows=H, out_cols=2 * W, layout=(1, 2, 1, 0, 0))
    check_maps(got, ref)
    for g, r, (img, _) in zip(got, ref, inputs(shape, fmt, 2 * W)):
        assert np.array_equal(g[2], quilt_ref([r[1], img[:, :W]], 2, 1, 0, 0, H, 2 * W))


def test_the_eye_with_4_byte_pixels(gpu_ready, stm):
    """elem_sz 4 through the C calls, the two images through the quilt's area filter on tiles of the views' own size (the renderer
    hands on three bytes of a pixel, so the fourth is not visible from here)"""
    lib = stm.lib()
    shape, fmt, fill = "21x83", "u16", 1
    H, W = SHAPES[shape]
    lo, hi = LIMITS[fmt]
    ref = reference(shape, fmt, fill, elem_sz=4)
    p = _params(2)
    h = lib.stm_stream_create(H, W, W, H, 2 * W, 4, 2, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                              p.thresh_s, p.thresh_h)
    try:
        assert lib.stm_stream_set_layout(h, 1, 2, 1, 0, 1) == 0 and lib.stm_stream_input_depth(h, 3, lo, hi, fill, GATE) == 0
        off = (H * W * 4 + 15) // 16 * 16
        for k, (img, plane) in enumerate(inputs(shape, fmt, None, 4)):
            flat = np.zeros(off + plane.nbytes, np.uint8)
            flat[:img.size] = img.reshape(-1)
            flat[off:] = plane.view(np.uint8).reshape(-1)
            assert lib.stm_stream_submit(h, flat.ctypes.data_as(u8p)) == k
            dl, dr, out = np.empty((H, W), f32), np.empty((H, W), f32), np.empty((H, 2 * W, 4), np.uint8)
            assert lib.stm_stream_collect(h, dl.ctypes.data_as(f32p), dr.ctypes.data_as(f32p), out.ctypes.data_as(u8p)) == k
            assert np.array_equal(dl, ref[k][0]) and np.array_equal(dr, ref[k][2]), k
            want = quilt_ref([ref[k][1], img[..., :3]], 2, 1, 0, 1, H, 2 * W)
            assert np.array_equal(out[..., :3], want), (k, int((out[..., :3] != want).sum()), np.argwhere((out[..., :3] != want).any(axis=2))[:6].tolist())
    finally:
        lib.stm_stream_destroy(h)


# ----------------------------------------------------------------------------- 2. the frame
@pytest.mark.parametrize("stages", [3, 3 | LINEAR_WARP], ids=["0x3", "0x803"])
@pytest.mark.parametrize("shape,fmt,fill", [("9x37", "u8", 1), ("16x64", "f32", 0), ("21x83", "u16", 1), ("5x300", "u8", 0)])
def test_the_frame(gpu_ready, orc, shape, fmt, fill, stages):
    """the default settings, 8 views: the reference's interlacer on the views rendered from (img, img_r, disp_l, disp_r)"""
    H, W = SHAPES[shape]
    ref = reference(shape, fmt, fill)
    got = run_depth(shape, fmt, fill, stages=stages)
    check_maps(got, ref)
    for k in (0, 1, 2, 3, N - 1):  # eager, eager, capture, capture, replay
        ch = chain_of(orc, inputs(shape, fmt)[k][0], ref[k])
        want = orc.mux_multiview(chain_views(orc, ch, 8, bool(stages & LINEAR_WARP)), ANGLE, H, W)
        assert np.array_equal(got[k][2], want), (k, int((got[k][2] != want).sum()))


# ----------------------------------------------------------------------------- 3. the settings reach it
def test_lens_mode_3_with_linear_warps(gpu_ready, orc):
    shape, fmt, fill = "16x64", "u8", 1
    H, W = SHAPES[shape]
    ref = reference(shape, fmt, fill)
    lens = (3,) + PANEL
    got = run_depth(shape, fmt, fill, stages=3 | LINEAR_WARP, lens=lens)
    check_maps(got, ref)
    for k in (0, 3, N - 1):
        want = render_lens_ref(orc, chain_of(orc, inputs(shape, fmt)[k][0], ref[k]), 8, lens, True, H, W)
        assert np.array_equal(got[k][2], want), (k, int((got[k][2] != want).sum()))


def test_quilt_with_a_manual_depth_budget(gpu_ready, orc):
    shape, fmt, fill = "21x83", "u16", 0
    ref = reference(shape, fmt, fill)
    Ho, Wo = 45, 170
    got = run_depth(shape, fmt, fill, out_rows=Ho, out_cols=Wo, layout=(1, 4, 2, 1, 1), depth=(0.6, 1.5))
    check_maps(got, ref)
    for k in (0, 3, N - 1):
        want = render_quilt_ref(orc, chain_of(orc, inputs(shape, fmt)[k][0], ref[k]), 8, 4, 2, 1, 1, Ho, Wo, False, depth=(0.6, 1.5))
        assert np.array_equal(got[k][2], want), (k, int((got[k][2] != want).sum()))


def test_automatic_depth_budget(gpu_ready, orc):
    """stm_stream_depth against depth_fit_ref chained over the frames, the frame against the render at the fitted numbers"""
    shape, fmt, fill = "16x64", "u8", 1
    ref = reference(shape, fmt, fill)
    lo, hi, mg, clip, rate = -1.5, 2.0, 1.5, 20, 0.5
    Ho, Wo = 40, 130
    got = run_depth(shape, fmt, fill, collect=lambda fs: fs.depth(), out_rows=Ho, out_cols=Wo, layout=(1, 4, 2, 2, 1),
                    depth_auto=(lo, hi, mg, clip, rate))
    check_maps(got, ref)
    state = np.zeros(4, f32)
    for k, (g, r) in enumerate(zip(got, ref)):
        state = depth_fit_ref(r[0], r[2], lo, hi, mg, clip, rate, state)
        assert g[3] == (float(state[1]), float(state[2])), (k, g[3], state)
        if k in (0, 3, N - 1):
            want = render_quilt_ref(orc, chain_of(orc, inputs(shape, fmt)[k][0], r), 8, 4, 2, 2, 1, Ho, Wo, False,
                                    depth=(state[1], state[2]))
            assert np.array_equal(g[2], want), (k, int((g[2] != want).sum()))
    assert state[1] != 1 and state[1] != mg  # a fit that neither bound decides


def test_overlay(gpu_ready, orc):
    from stm_amd import video
    shape, fmt, fill = "16x64", "f32", 0
    H, W = SHAPES[shape]
    lo, hi = LIMITS[fmt]
    base = run_depth(shape, fmt, fill)
    ov = random_overlay(11, 5, 9)
    shift = subpixel_shift_ref(orc, H, W, 8, 3, ANGLE)
    fs = video.FrameStream(H, W, _params(), depth_input=(fmt, lo, hi, fill, GATE), overlay=(5, 9))
    try:
        fs.overlay(ov, 20, 4, -3.5)
        for k, (img, plane) in enumerate(inputs(shape, fmt)):
            assert fs.submit_depth(img, plane) == k
            r = fs.collect()
            want = overlay_ref(base[k][2], ov, 20, 4, -3.5, shift)
            assert np.array_equal(r[3], want) and not np.array_equal(want, base[k][2]), k
    finally:
        fs.close()


def test_maps_leave_as_u8_planes(gpu_ready):
    shape, fmt, fill = "21x83", "u16", 1
    ref = reference(shape, fmt, fill)
    base = run_depth(shape, fmt, fill)
    got = run_depth(shape, fmt, fill, maps=("u8", "both", 10.0, -10.0))
    for k, (g, r, b) in enumerate(zip(got, ref, base)):
        assert g[0].dtype == np.uint8 and np.array_equal(g[0], plane_ref(r[0], "u8", 10.0, -10.0)), k
        assert np.array_equal(g[1], plane_ref(r[2], "u8", 10.0, -10.0)) and np.array_equal(g[2], b[2]), k


def test_cut_and_automatic_active_area_see_the_image_as_the_left_eye(gpu_ready):
    """stm_stream_cut and stm_stream_active equal those of a stereo stream fed [img | img]: bars of three and two rows, another
    picture from frame 4 on"""
    from stm_amd import video
    shape, fmt, fill = "16x64", "u8", 0
    H, W = SHAPES[shape]
    frames = []
    for k, (_, plane) in enumerate(inputs(shape, fmt)):
        img = scene_image(H, W).copy()
        if k >= 4:  # the same picture at a quarter of the contrast: every cell's histogram moves into four bins
            img = (img >> 2) + 100
        img[:3] = 0
        img[H - 2:] = 0
        frames.append((img, plane))
    kw = dict(cut=True, active_auto=(24, 10, 300, 2), active_fill=0.0)
    got = run_depth(shape, fmt, fill, frames=frames, collect=lambda fs: (fs.cut(), fs.active()), **kw)
    fs = video.FrameStream(H, W, _params(), **kw)
    try:
        for k, (img, _) in enumerate(frames):
            assert fs.submit(np.concatenate([img, img], axis=1)) == k
            assert fs.collect() is not None
            assert got[k][3] == (fs.cut(), fs.active()), (k, got[k][3], fs.cut(), fs.active())
    finally:
        fs.close()
    assert [g[3][0][0] for g in got] == [1, 0, 0, 0, 1, 0, 0]
    assert got[-1][3][1][:4] != (0, H, 0, W)  # the bars were found
    lo, hi = LIMITS[fmt]
    for g, (img, plane) in zip(got, frames):  # the active fill reaches both maps
        top, bottom = g[3][1][:2]
        dl = decode_ref(plane, fmt, lo, hi)
        assert not g[0][:top].any() and not g[1][bottom:].any() and np.array_equal(g[0][top:bottom], dl[top:bottom])


# ----------------------------------------------------------------------------- 4. round trip
def test_round_trip_through_the_planes_of_stream_maps(gpu_ready):
    """a stereo stream's own u16 left planes, with its left halves, through a depth stream: disp_l is the decoded plane"""
    from stm_amd import device_api as dev, video
    H, W = SEQ["H"], SEQ["W"]
    p = dev.FrameParams(num_disp=SEQ["D"], zero_disp=SEQ["zd"], usd=SEQ["usd"], lsd=SEQ["lsd"])
    lo, hi = float(SEQ["zd"] - SEQ["D"]), float(SEQ["zd"])
    seq = mixed_sequence(N)
    fs = video.FrameStream(H, W, p, maps=("u16", "left", lo, hi))
    planes = []
    try:
        for k, f in enumerate(seq):
            assert fs.submit(f) == k
            planes.append(np.array(fs.collect()[1]))
    finally:
        fs.close()
    assert len(set(pl.tobytes() for pl in planes)) > 1 and all(0 < len(np.unique(pl)) for pl in planes)
    frames = [(np.ascontiguousarray(f[:, :W]), pl) for f, pl in zip(seq, planes)]
    got = run_depth((H, W), "u16", 1, frames=frames, limits=(lo, hi), params=p)
    for k, (g, (img, pl)) in enumerate(zip(got, frames)):
        dl = decode_ref(pl, "u16", lo, hi)
        assert np.array_equal(g[0], dl), k
        assert np.array_equal(plane_ref(g[0], "u16", lo, hi), pl), k
        assert np.array_equal(g[1], eye_ref(img, dl, 1, GATE)[1]), k


# ----------------------------------------------------------------------------- 4b. disparities far beyond the row
FAR = (-4096.0, 4096.0)


@functools.lru_cache(maxsize=None)
def far_frames(shape):
    """the scene with +-4096 and +-W planted at columns 0, 1, W / 2, W - 2 and W - 1, the signs and rows moving with the frame"""
    H, W = SHAPES[shape]
    img = scene_image(H, W)
    img.setflags(write=False)
    vals = [4096.0, -4096.0, float(W), float(-W)]
    frames = []
    for k in range(N):
        d = scene_disp(H, W, k)
        for j, c in enumerate((0, 1, W // 2, W - 2, W - 1)):
            d[(2 * j + k) % H, c] = vals[(j + k) % 4]
            d[(2 * j + k + 1) % H, c] = vals[(j + k + 2) % 4]
        d.setflags(write=False)
        frames.append((img, d))
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def far_reference(shape, fill):
    out = []
    for img, plane in far_frames(shape):
        dl = decode_ref(plane, "f32", *FAR)
        out.append((dl,) + eye_ref(img, dl, fill, GATE))
    return tuple(out)


@pytest.mark.parametrize("shape,fill", [("9x37", 1), ("5x300", 0)])
def test_disparities_far_beyond_the_row(gpu_ready, orc, shape, fill):
    """An f32 depth stream with limits (-4096, 4096), the widest a plane's values survive step A: the only public route by which maps
    with |d| far beyond W reach stm_k_eye, stm_k_hitmask_rows and the fused renderer.  The maps and img_r against eye_ref, the
    frame against the chain.  Those kernels add before they clamp the column (x + (int)d, x + (int)(d * +-1)), in 32 bits: after
    step A |d| <= 4096, and x < W, so |x + (int)d| <= W + 4096, which is below 2^31 for every width a frame can have; nothing
    saturates and no sum wraps.  (The per-stage calls take any map: tests/test_gpu_map_edges.py.)"""
    H, W = SHAPES[shape]
    frames, ref = far_frames(shape), far_reference(shape, fill)
    x = np.arange(W)[None, :]
    for r in ref:  # conditions on the inputs: pixels land beyond both ends of the row, from both maps
        assert r[4]["clamped_left"] > 0 and r[4]["clamped_right"] > 0, r[4]
        assert (r[0] == 4096).any() and (r[0] == -4096).any() and (r[0] == W).any() and (r[0] == -W).any()
        for sd in (r[0].astype(np.int64), -r[2].astype(np.int64)):  # the hit maps' shifts: disp_l and -disp_r
            assert ((x + sd) < 0).any() and ((x + sd) > W - 1).any()
    order = 0 if fill == 0 else 2
    got = run_depth(shape, "f32", fill, frames=frames, limits=FAR, params=_params(2), out_rows=H, out_cols=2 * W,
                    layout=(1, 2, 1, order, 0))
    check_maps(got, ref)
    for k, (g, r, (img, _)) in enumerate(zip(got, ref, frames)):
        want = quilt_ref([r[1], img], 2, 1, order, 0, H, 2 * W)
        assert np.array_equal(g[2], want), (k, "img_r", int((g[2] != want).sum()))
    got = run_depth(shape, "f32", fill, frames=frames, limits=FAR, stages=3)
    check_maps(got, ref)
    for k in (0, 2, N - 1):  # eager, capture, replay
        want = orc.mux_multiview(chain_views(orc, chain_of(orc, frames[k][0], ref[k]), 8, False), ANGLE, H, W)
        assert np.array_equal(got[k][2], want), (k, int((got[k][2] != want).sum()))


# ----------------------------------------------------------------------------- 5. the refusals, in both directions
def test_refusals_leave_the_stream_as_it_was(gpu_ready, stm, orc):
    from stm_amd import video
    lib = stm.lib()
    shape, fmt, fill = "9x37", "u8", 1
    H, W = SHAPES[shape]
    lo, hi = LIMITS[fmt]
    ref = reference(shape, fmt, fill)
    nan, inf = float("nan"), float("inf")
    lib.stm_set_error_mode(1)
    streams = []

    def stream(**kw):
        streams.append(video.FrameStream(H, W, _params(), **kw))
        return streams[-1]

    def refused(call, *words):
        lib.stm_d_filter_median(None, 0, 0)  # plant a known message
        assert call() == -1
        err = lib.stm_last_error()
        assert all(wd in err for wd in words), err
    try:
        fs = stream(depth_input=(fmt, lo, hi, fill, GATE))
        sd = lib.stm_stream_input_depth
        me = b"stream_input_depth:"
        for bad in (1, 4, -2):
            refused(lambda: sd(fs._h, bad, lo, hi, 0, 0.0), me, b"format")
        for f in (0, 2, 3):
            for a, b in ((3.0, 3.0), (3.0, 3.0 + 1.0 / 128.0), (nan, 1.0), (1.0, nan), (inf, 0.0), (0.0, -inf), (5000.0, 0.0), (0.0, -5000.0)):
                refused(lambda: sd(fs._h, f, a, b, 0, 0.0), me, b"lo", b"hi")
            refused(lambda: sd(fs._h, f, lo, hi, 2, 0.0), me, b"fill")
            refused(lambda: sd(fs._h, f, lo, hi, -1, 0.0), me, b"fill")
            for g in (nan, inf, -0.5, 5000.0):
                refused(lambda: sd(fs._h, f, lo, hi, 1, g), me, b"gate")
            assert sd(fs._h, f, lo, hi, 0, nan) == 0  # fill 0 does not look at the gate
        assert sd(fs._h, 2, lo, hi, fill, GATE) == 0  # ... and back to the test's setting
        # the other direction: the settings of a stereo pair and its matcher name their own entry and the depth input
        other = [("stream_set_input:", lambda: lib.stm_stream_set_input(fs._h, 1, 0)),
                 ("stream_set_input:", lambda: lib.stm_stream_set_input(fs._h, 0, 0)),
                 ("stream_set_packing:", lambda: lib.stm_stream_set_packing(fs._h, 1, 0, 0, 0)),
                 ("stream_set_match_size:", lambda: lib.stm_stream_set_match_size(fs._h, 5, 19, 0.5)),
                 ("stream_set_align:", lambda: lib.stm_stream_set_align(fs._h, 1, 0.5, 0.0, 0.0)),
                 ("stream_set_balance:", lambda: lib.stm_stream_set_balance(fs._h, 2, None)),
                 ("stream_set_stages:", lambda: lib.stm_stream_set_stages(fs._h, 3 | 0x200)),
                 ("stream_set_stages:", lambda: lib.stm_stream_set_stages(fs._h, 3 | 0x2000))]
        for name, call in other:
            refused(call, name.encode(), b"depth input")
        assert lib.stm_stream_set_stages(fs._h, 3 | 0x800) == 0 and lib.stm_stream_set_stages(fs._h, 3) == 0
        # after all of that the stream still produces frame 0, and refuses the call after it
        img, plane = inputs(shape, fmt)[0]
        assert fs.submit_depth(img, plane) == 0
        refused(lambda: sd(fs._h, 2, lo, hi, 0, 0.0), me, b"first submit")
        refused(lambda: sd(fs._h, -1, 0.0, 0.0, 0, 0.0), me, b"first submit")
        refused(lambda: sd(fs._h, 7, lo, hi, 0, 0.0), me, b"format")  # the broken argument wins
        k, dl, dr, out = fs.collect()
        assert k == 0 and np.array_equal(dl, ref[0][0]) and np.array_equal(dr, ref[0][2])
        want = orc.mux_multiview(chain_views(orc, chain_of(orc, img, ref[0]), 8, False), ANGLE, H, W)
        assert np.array_equal(out, want)
        # a stream that already has what a depth frame does not go with
        for kw, word in ((dict(input_format="nv12"), b"NV12"), (dict(packing=(2, 0, 0, 0)), b"packing"), (dict(match=(5, 19, 0.5)), b"match size"),
                         (dict(align=(0.5, 0.0, 0.0)), b"alignment"),
                         (dict(balance=np.tile(np.arange(256, dtype=np.uint8)[::-1], (3, 1))), b"balance"),
                         (dict(stages=3 | 0x400), b"stages"), (dict(stages=3 | 0x2000), b"stages")):
            if "input_format" in kw:  # NV12 needs even sizes
                streams.append(video.FrameStream(10, 38, _params(), **kw))
                s = streams[-1]
            else:
                s = stream(**kw)
            refused(lambda: sd(s._h, 2, lo, hi, 0, 0.0), me, word)
            assert sd(s._h, -1, 0.0, 0.0, 0, 0.0) == 0  # off is what such a stream already is
        wide = video.FrameStream(2, 8200, _params())
        streams.append(wide)
        refused(lambda: sd(wide._h, 2, lo, hi, 0, 0.0), me, b"num_cols", b"8192")
        with pytest.raises(ValueError, match="stm_stream_input_depth"):
            video.FrameStream(H, W, _params(), depth_input=("u8", 2.0, 2.0))
        # switched on and off again: a stereo stream as it was
        s = stream()
        assert sd(s._h, 3, lo, hi, 1, GATE) == 0 and sd(s._h, -1, 0.0, 0.0, 0, 0.0) == 0
        assert lib.stm_stream_set_stages(s._h, 3 | 0x200) == 0
    finally:
        lib.stm_set_error_mode(0)
        for s in streams:
            s.close()


def test_the_widest_row(gpu_ready):
    """num_cols 8192: the keys take 64 KiB of LDS and the launch opts in to more than the default limit"""
    from stm_amd import video
    H, W = 2, 8192
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    plane = rng.randint(0, 256, size=(H, W)).astype(np.uint8)
    plane[:, 4000:4200] = 255
    dl = decode_ref(plane, "u8", -20.0, 20.0)
    img_r, dr, holes, _ = eye_ref(img, dl, 1, GATE)
    fs = video.FrameStream(H, W, _params(2), H, 2 * W, layout=(1, 2, 1, 0, 0), depth_input=("u8", -20.0, 20.0, 1, GATE))
    try:
        for k in range(3):
            assert fs.submit_depth(img, plane) == k
            r = fs.collect()
            assert np.array_equal(r[1], dl) and np.array_equal(r[2], dr) and np.array_equal(r[3][:, :W], img_r), k
    finally:
        fs.close()
    assert holes.any()


# ----------------------------------------------------------------------------- 6. a stream without the call
def _stereo_digest(switch=False):
    """sha256 over the maps and frames of a plain stereo stream; switch: depth input switched on and off again before the first frame"""
    from stm_amd import video
    import test_gpu_stream_maps as t
    H, W = t.SHAPES["24x40"][:2]
    fs = video.FrameStream(H, W, t._params("24x40"))
    h = hashlib.sha256()
    try:
        if switch:
            fs.set_depth_input("u16", -3.0, 9.0, 1, 0.25)
            fs.set_depth_input("off")
        for k, f in enumerate(t.frames_of("24x40")):
            assert fs.submit(f) == k
            for a in fs.collect()[1:]:
                h.update(np.ascontiguousarray(a).tobytes())
    finally:
        fs.close()
    return h.hexdigest()


def test_a_stream_without_the_call_is_a_fresh_process_stream(gpu_ready):
    """after depth streams have run in this process, a stereo stream -- untouched, or with the depth input switched on and off again --
    gives the bytes of a stereo stream in a process that never heard of the setting"""
    run_depth("9x37", "u8", 1)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_depth_input as t\n"
            "print('digest', t._stereo_digest())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "digest " in r.stdout, r.stdout + r.stderr
    fresh = r.stdout.strip().split("digest ")[-1]
    assert _stereo_digest() == fresh and _stereo_digest(switch=True) == fresh
