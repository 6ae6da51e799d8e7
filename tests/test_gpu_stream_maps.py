"""The map formats of a frame stream on the GPU (stm_stream_maps).  The float maps F come from a format-0
stream over the same frames -- other tests pin that stream to the oracle --, once per configuration and shared; the planes of a u8 /
u16 stream must equal test_stream_maps_ref.plane_ref(F, ...) bit for bit and its frames the format-0 stream's byte for byte.  Seven
frames per stream: both slots run eager, capture their graph and replay it.  Shapes: 24 x 40 (HW a multiple of 16), 37 x 83 (HW =
3071: a u8 tail of 15 codes, a u16 tail of 7, and with both planes a right plane at an odd byte offset) and 19 x 67 (HW = 1273: the
right plane starts 9 bytes (u8) or 2 bytes (u16) past a 16-byte boundary of the slot's buffer)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_nv12_ref import nv12_frame
from test_stream_maps_ref import DTYPE, MAXCODE, plane_ref
from test_temporal_ref import SEQ, mixed_sequence

pytestmark = pytest.mark.gpu

N = 7
# H, W, num_disp, zero_disp, usd, lsd
SHAPES = {"24x40": (24, 40, 16, 8, 17, 8), "37x83": (37, 83, 24, 12, 17, 8), "19x67": (19, 67, 21, 10, 17, 8),
          "40x72": (SEQ["H"], SEQ["W"], SEQ["D"], SEQ["zd"], SEQ["usd"], SEQ["lsd"])}
SUBPIXEL, GUIDED_UP, TEMPORAL = 0x200, 0x1000, 0x2000
f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def _params(shape):
    from stm_amd import device_api as dev
    _, _, D, zd, usd, lsd = SHAPES[shape]
    return dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd)


_FRAMES = {}


def frames_of(shape):
    """N side-by-side frames of one synthetic scene: a flat rectangle moves two pixels a frame over both halves under noise of +-2,
    so the maps differ from frame to frame and a temporal step finds pixels on both sides of its gates"""
    if shape == "40x72":
        return mixed_sequence(N)
    if shape not in _FRAMES:
        from stm_amd import synth
        H, W, D, zd = SHAPES[shape][:4]
        base, _ = synth.sbs_frame(H, W, D, zd)
        rng = np.random.RandomState(H * 1000 + W)
        out = []
        for k in range(N):
            f = base.copy()
            for x0 in (3 + 2 * k, W + 1 + 2 * k):
                f[H // 4:H // 4 + H // 3, x0:x0 + W // 5] = (200, 60, 30)
            out.append(np.clip(f.astype(np.int32) + rng.randint(-2, 3, size=f.shape), 0, 255).astype(np.uint8))
        _FRAMES[shape] = out
    return _FRAMES[shape]


def run_stream(shape, frames=None, view=False, **kw):
    """the frames through a FrameStream(**kw), two in flight; returns [(disp_l or plane_l or None, ... right, frame)] as copies"""
    from stm_amd import video
    H, W = SHAPES[shape][:2]
    fs = video.FrameStream(H, W, _params(shape), **kw)
    try:
        got, pending = [], 0

        def take():
            r = fs.collect_view() if view else fs.collect()
            assert r is not None and r[0] == len(got)
            got.append(tuple(None if a is None else np.array(a) for a in r[1:]))
        for f in (frames_of(shape) if frames is None else frames):
            if pending == 2:
                take()
                pending -= 1
            assert fs.submit(f) >= 0
            pending += 1
        while pending:
            take()
            pending -= 1
    finally:
        fs.close()
    return got


_FLOAT = {}


def float_stream(shape, key="", frames=None, **kw):
    """the format-0 stream of a configuration, computed once and never modified"""
    if (shape, key) not in _FLOAT:
        got = run_stream(shape, frames, **kw)
        for g in got:
            for a in g:
                a.setflags(write=False)
            assert g[0].dtype == np.float32 and np.isfinite(g[0]).all() and np.isfinite(g[1]).all()
        _FLOAT[(shape, key)] = got
    return _FLOAT[(shape, key)]


def limits_of(F, reverse):
    """lo, hi: the 25th and the 75th percentile of the float maps themselves, so both clamps fire (a condition on the inputs)"""
    allv = np.concatenate([np.stack([g[0], g[1]]).reshape(-1) for g in F])
    a, b = np.float32(np.percentile(allv, 25)), np.float32(np.percentile(allv, 75))
    assert np.isfinite([a, b]).all() and float(b) - float(a) >= 1.0 / 64.0, (a, b)
    return (float(b), float(a)) if reverse else (float(a), float(b))


def planes_check(shape, fmt, which, reverse, key="", frames=None, view=False, **kw):
    """one u8 / u16 stream against the format-0 stream of the same configuration"""
    F = float_stream(shape, key, frames, **kw)
    lo, hi = limits_of(F, reverse)
    got = run_stream(shape, frames, view=view, maps=(fmt, which, lo, hi), **kw)
    assert len(got) == len(F) == N
    codes = []
    for k, (g, want) in enumerate(zip(got, F)):
        for v, name in ((0, "left"), (1, "right")):
            if which in (name, "both"):
                assert g[v] is not None and g[v].dtype == DTYPE[fmt] and g[v].shape == want[v].shape
                ref = plane_ref(want[v], fmt, lo, hi)
                assert np.array_equal(g[v], ref), (shape, fmt, which, reverse, k, name, int((g[v] != ref).sum()))
                codes.append(g[v])
            else:
                assert g[v] is None, (k, name)
        assert np.array_equal(g[2], want[2]), (shape, fmt, which, reverse, k, "frame")
    codes = np.concatenate([c.reshape(-1) for c in codes])
    assert (codes == 0).any() and (codes == MAXCODE[fmt]).any() and ((codes > 0) & (codes < MAXCODE[fmt])).any()
    return F


# ----------------------------------------------------------------------------- 1. the planes, bit for bit
@pytest.mark.parametrize("reverse", [False, True], ids=["lo<hi", "lo>hi"])
@pytest.mark.parametrize("which", ["left", "right", "both"])
@pytest.mark.parametrize("fmt", ["u8", "u16"])
@pytest.mark.parametrize("shape", ["24x40", "37x83", "19x67"])
def test_planes_are_the_quantised_float_maps(gpu_ready, shape, fmt, which, reverse):
    planes_check(shape, fmt, which, reverse)


def test_views_of_the_planes(gpu_ready):
    """the zero-copy collect on the same data (run_stream copies each view at once)"""
    planes_check("37x83", "u8", "both", False, view=True)
    planes_check("19x67", "u16", "right", True, view=True)


def test_fractional_maps_round(gpu_ready):
    """sub-pixel maps: the codes come from rounding, not from integers scaled"""
    F = planes_check("37x83", "u16", "both", False, key="subpixel", stages=3 | SUBPIXEL)
    assert any((g[0] != np.floor(g[0])).any() for g in F)
    planes_check("37x83", "u8", "both", True, key="subpixel", stages=3 | SUBPIXEL)


def test_temporal_history_stays_float(gpu_ready):
    """0x2000: frame k is stabilised against frame k - 1's float maps, which the plane stream never downloads: its planes equal
    the quantised maps of the format-0 temporal stream on every frame -- quantised history would drift from the second frame on"""
    F = planes_check("24x40", "u8", "both", False, key="temporal", stages=3 | TEMPORAL)
    plain = float_stream("24x40")
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(F[1:], plain[1:]))  # the step acts
    planes_check("37x83", "u16", "left", True, key="temporal", stages=3 | TEMPORAL)


def test_nv12_input(gpu_ready):
    from stm_amd import synth
    frames = [nv12_frame(*synth.bgr_to_nv12(f)) for f in frames_of("24x40")]
    planes_check("24x40", "u8", "both", False, key="nv12", frames=frames, input_format="nv12")


def test_match_size_with_guided_upsampling(gpu_ready):
    """the reduced-resolution frame: planes of the full-resolution maps the stream hands out, H x W"""
    H, W = SHAPES["40x72"][:2]
    planes_check("40x72", "u16", "both", False, key="match", match=(H // 2, W // 2, 0.5), stages=3 | GUIDED_UP)


def test_quilt_layout(gpu_ready):
    planes_check("24x40", "u8", "right", True, key="quilt", layout=(1, 4, 2, 3, 1))


def test_without_graphs_in_a_child_process(gpu_ready):
    """STM_STREAM_GRAPH is read when the stream is created: a fresh child process, every launch eager"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_stream_maps as t\n"
            "t.planes_check('37x83', 'u8', 'both', False)\n"
            "t.planes_check('19x67', 'u16', 'both', True)\n"
            "print('ok')\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, STM_STREAM_GRAPH="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ----------------------------------------------------------------------------- 2. no maps
def test_format_none(gpu_ready, stm):
    from stm_amd import video
    lib = stm.lib()
    shape = "37x83"
    F = float_stream(shape)
    got = run_stream(shape, maps="none")
    assert all(g[0] is None and g[1] is None and np.array_equal(g[2], w[2]) for g, w in zip(got, F))
    H, W = SHAPES[shape][:2]
    fs = video.FrameStream(H, W, _params(shape), maps=("none",))
    lib.stm_set_error_mode(1)
    try:
        assert fs.submit(frames_of(shape)[0]) == 0
        dl = np.full((H, W), 7.0, np.float32)
        out = np.zeros((H, W, 3), np.uint8)
        for args in ((dl.ctypes.data_as(f32p), None), (None, dl.ctypes.data_as(f32p))):
            lib.stm_d_filter_median(None, 0, 0)  # plant a known message
            assert lib.stm_stream_collect(fs._h, *args, out.ctypes.data_as(u8p)) == -1
            err = lib.stm_last_error()
            assert b"stream_collect:" in err and b"stm_stream_maps" in err, err
        pl, po = f32p(), u8p()
        assert lib.stm_stream_collect_view(fs._h, C.byref(pl), None, C.byref(po)) == -1 and b"stream_collect_view:" in lib.stm_last_error()
        plane = np.zeros((H, W), np.uint8)
        assert lib.stm_stream_collect_maps(fs._h, plane.ctypes.data, None, out.ctypes.data_as(u8p)) == -1
        assert b"stream_collect_maps:" in lib.stm_last_error() and b"plane_l" in lib.stm_last_error()
        assert (dl == 7.0).all() and not out.any() and not plane.any()  # nothing was written, nothing consumed:
        assert lib.stm_stream_collect(fs._h, None, None, out.ctypes.data_as(u8p)) == 0  # the frame is still there
        assert np.array_equal(out, F[0][2])
        assert fs.submit(frames_of(shape)[1]) == 1
        vl, vr = C.c_void_p(1), C.c_void_p(1)
        assert lib.stm_stream_collect_maps_view(fs._h, C.byref(vl), C.byref(vr), C.byref(po)) == 1
        assert vl.value is None and vr.value is None
        assert np.array_equal(np.ctypeslib.as_array(po, shape=(H, W, 3)), F[1][2])
    finally:
        lib.stm_set_error_mode(0)
        fs.close()


# ----------------------------------------------------------------------------- 3. how long a view lasts
def test_views_last_until_the_frame_after_the_next_is_submitted(gpu_ready):
    from stm_amd import video
    shape = "37x83"
    H, W = SHAPES[shape][:2]
    F = float_stream(shape)
    lo, hi = limits_of(F, False)
    want = [(plane_ref(g[0], "u16", lo, hi), plane_ref(g[1], "u16", lo, hi), g[2]) for g in F]
    frames = frames_of(shape)
    fs = video.FrameStream(H, W, _params(shape), maps=("u16", "both", lo, hi))
    try:
        def same(view, k):
            return view[0] == k and all(np.array_equal(a, b) for a, b in zip(view[1:], want[k]))
        assert fs.submit(frames[0]) == 0 and fs.submit(frames[1]) == 1
        held = {0: fs.collect_view()}
        assert same(held[0], 0)
        for k in range(2, N):
            held[k - 1] = fs.collect_view()              # frame k - 1 is done; frame k - 2's views are still untouched:
            assert same(held[k - 1], k - 1) and same(held[k - 2], k - 2)
            assert fs.submit(frames[k]) == k             # frame k takes frame k - 2's slot: those views are void from here on
            del held[k - 2]
            assert same(held[k - 1], k - 1)              # the other slot's stay valid while frame k is computed and downloaded
        last = fs.collect_view()
        assert same(last, N - 1) and same(held[N - 2], N - 2)
    finally:
        fs.close()


# ----------------------------------------------------------------------------- 4. what the setter and the collects refuse
def test_refusals_leave_the_stream_as_it_was(gpu_ready, stm):
    from stm_amd import video
    lib = stm.lib()
    shape = "24x40"
    H, W = SHAPES[shape][:2]
    F = float_stream(shape)
    frames = frames_of(shape)
    fs = video.FrameStream(H, W, _params(shape))
    lib.stm_set_error_mode(1)
    try:
        def refused(call, *words):
            lib.stm_d_filter_median(None, 0, 0)  # plant a known message
            assert call() == -1
            err = lib.stm_last_error()
            assert all(wd in err for wd in words), err
        sm = lib.stm_stream_maps
        nan, inf = float("nan"), float("inf")
        refused(lambda: sm(fs._h, 4, 2, 0.0, 16.0), b"stream_maps:", b"format")
        refused(lambda: sm(fs._h, -1, 2, 0.0, 16.0), b"stream_maps:", b"format")
        for fmt in (2, 3):
            refused(lambda: sm(fs._h, fmt, 3, 0.0, 16.0), b"stream_maps:", b"which")
            refused(lambda: sm(fs._h, fmt, -1, 0.0, 16.0), b"stream_maps:", b"which")
            for lo, hi in ((3.0, 3.0), (3.0, 3.0 + 1.0 / 128.0), (nan, 1.0), (1.0, nan), (inf, 0.0), (0.0, -inf), (5000.0, 0.0), (0.0, -5000.0)):
                refused(lambda: sm(fs._h, fmt, 2, lo, hi), b"stream_maps:", b"lo", b"hi")
        assert sm(fs._h, 0, 7, nan, nan) == 0 and sm(fs._h, 1, -3, inf, inf) == 0  # formats 0 and 1 look at nothing else
        assert sm(fs._h, 3, 1, 4096.0, -4096.0) == 0 and sm(fs._h, 2, 0, 1.0, 1.0 + 1.0 / 64.0) == 0  # the rules' own edges
        refused(lambda: sm(fs._h, 2, 5, 0.0, 16.0), b"stream_maps:", b"which")  # ... and a refusal keeps the format set before it
        assert sm(fs._h, 0, 0, 0.0, 0.0) == 0  # back to the default, whose pinned float buffers exist again
        assert fs.submit(frames[0]) == 0
        refused(lambda: sm(fs._h, 2, 2, 0.0, 16.0), b"stream_maps:", b"first submit")
        refused(lambda: sm(fs._h, 0, 2, 0.0, 16.0), b"stream_maps:", b"first submit")
        refused(lambda: sm(fs._h, 9, 2, 0.0, 16.0), b"stream_maps:", b"format")  # the broken argument wins
        plane, out = np.zeros((H, W), np.uint16), np.zeros((H, W, 3), np.uint8)
        refused(lambda: lib.stm_stream_collect_maps(fs._h, plane.ctypes.data, None, out.ctypes.data_as(u8p)), b"stream_collect_maps:", b"format is 0")
        vl, vr, po = C.c_void_p(), C.c_void_p(), u8p()
        refused(lambda: lib.stm_stream_collect_maps_view(fs._h, C.byref(vl), C.byref(vr), C.byref(po)), b"stream_collect_maps_view:", b"format is 0")
        assert not plane.any() and not out.any()
        # the stream still works, and gives the default results
        got = [fs.collect()]
        for k in range(1, N):
            assert fs.submit(frames[k]) == k
            got.append(fs.collect())
        for k, (g, w) in enumerate(zip(got, F)):
            assert g[0] == k and g[1].dtype == np.float32 and all(np.array_equal(a, b) for a, b in zip(g[1:], w)), k
        with pytest.raises(ValueError, match="stm_stream_maps"):
            video.FrameStream(H, W, _params(shape), maps=("u8", "both", 2.0, 2.0))
    finally:
        lib.stm_set_error_mode(0)
        fs.close()
