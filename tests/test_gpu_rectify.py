"""The rectification on the GPU (stm_rectify, stm_d_rectify, stm_rectify_coords, stm_stream_rectify), bit for bit against the numpy
statement in tests/test_rectify_ref.py.  A stream with the setting on is compared with the same stream without it on the statement's
rectified frames."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_nv12_ref import nv12_frame
from test_packing_ref import unpack_nv12_ref, unpack_ref
from test_rectify_ref import SHAPES, camera, case_records, coords_ref, identity, quv_ref, rectify_ref, rot_z, texture

pytestmark = pytest.mark.gpu

T = 0x2000
FILL = 0x77
D, ZD = 16, 8
f32p = C.POINTER(C.c_float)


@pytest.fixture(autouse=True)
def _settings_at_their_defaults_afterwards(gpu_ready):
    from stm_amd import device_api as dev
    yield
    assert dev.get_align()[0] == 0 and dev.get_packing() == dev.PACKING_OFF, "a test left a setting of the thread on"


@pytest.fixture
def lib(stm, gpu_ready):
    import torch
    l = stm.lib()
    l.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return l


def _rp(rec):
    rec = np.ascontiguousarray(rec, dtype=np.float32)
    return rec, rec.ctypes.data_as(f32p)


# ------------------------------------------------------------------------------------------------------- 1. the stage and the tap
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_rectify_device(lib, shape):
    """every record x both borders x 3- and 4-byte pixels, caller buffers at byte offsets 0 .. 3 (input and output differently), the
    bytes past a pixel's third left alone, nothing outside the output written; the identity returns the input's bytes"""
    from test_gpu_caller_buffers import Arena, P, read
    H, W = shape
    arena = Arena(True, nbytes=24 << 20)
    want = {}
    cases = []
    n = 0
    for E in (3, 4):
        img = texture(H, W, H * 1000 + W, E)
        for name, rec in case_records(H, W).items():
            r, pr = _rp(rec)
            for border in (0, 1):
                if (name, border) not in want:
                    want[(name, border)] = rectify_ref(img, rec, border)
                d_img = arena.put(img, n % 4)
                d_out = arena.put(np.full((H, W, E), FILL, np.uint8), (n // 4 + n + 1) % 4)
                lib.stm_d_rectify(P(d_out), P(d_img), pr, H, W, E, border)
                cases.append((name, border, E, img, d_out, n % 4, (n // 4 + n + 1) % 4))
                n += 1
    assert arena.intact(), shape
    assert {c[5] for c in cases} == {0, 1, 2, 3} and {c[6] for c in cases} == {0, 1, 2, 3}
    for name, border, E, img, d_out, oi, oo in cases:
        got = read(d_out, np.uint8, (H, W, E))
        assert np.array_equal(got[:, :, :3], want[(name, border)]), (name, border, E, oi, oo)
        assert (got[:, :, 3:] == FILL).all(), (name, border, E)
        if name == "identity":
            assert np.array_equal(got[:, :, :3], img[:, :, :3])


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_rectify_coords(gpu_ready, shape):
    from stm_amd import host_api as api
    H, W = shape
    for name, rec in case_records(H, W).items():
        assert np.array_equal(api.rectify_coords(rec, H, W), quv_ref(rec, H, W)), name


def test_rectify_host(gpu_ready):
    from stm_amd import host_api as api
    for (H, W, E) in [(5, 65, 3), (33, 300, 4), (9, 37, 4)]:
        img = texture(H, W, 9, E)
        for name, rec in case_records(H, W).items():
            for border in (0, 1):
                got = api.rectify(img, rec, border)
                assert np.array_equal(got[:, :, :3], rectify_ref(img, rec, border)) and (got[:, :, 3:] == 0).all(), (name, border, H, W, E)


def test_refusals_write_nothing(lib):
    import torch
    H, W, E = 5, 7, 3
    img = torch.from_numpy(texture(H, W, 1)).cuda()
    out = torch.full((H, W, E), FILL, dtype=torch.uint8, device="cuda")
    h_img = texture(H, W, 1)
    h_out = np.full((H, W, E), FILL, np.uint8)
    quv = np.full((H, W, 2), 5, np.int32)
    _, good = _rp(identity())
    recs = {}
    for k, v in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        r = identity()
        r[13 if k == "nan" else 2] = v
        recs[k] = _rp(r)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    ip = quv.ctypes.data_as(C.POINTER(C.c_int))
    lib.stm_set_error_mode(1)
    try:
        dev_cases = [((None, img.data_ptr(), good, H, W, E, 0), b"null"), ((out.data_ptr(), None, good, H, W, E, 0), b"null"),
                     ((out.data_ptr(), img.data_ptr(), None, H, W, E, 0), b"null"),
                     ((out.data_ptr(), img.data_ptr(), good, 0, W, E, 0), b"num_rows"), ((out.data_ptr(), img.data_ptr(), good, H, 0, E, 0), b"num_cols"),
                     ((out.data_ptr(), img.data_ptr(), good, 16385, W, E, 0), b"num_rows"),
                     ((out.data_ptr(), img.data_ptr(), good, H, 16385, E, 0), b"num_cols"),
                     ((out.data_ptr(), img.data_ptr(), good, H, W, 2, 0), b"elem_sz"), ((out.data_ptr(), img.data_ptr(), good, H, W, E, 2), b"border"),
                     ((out.data_ptr(), img.data_ptr(), good, H, W, E, -1), b"border"),
                     ((out.data_ptr(), img.data_ptr(), recs["nan"][1], H, W, E, 0), b"finite"),
                     ((out.data_ptr(), img.data_ptr(), recs["inf"][1], H, W, E, 0), b"finite"),
                     ((out.data_ptr(), img.data_ptr(), recs["-inf"][1], H, W, E, 1), b"finite"),
                     ((img.data_ptr() + 3 * W, img.data_ptr(), good, H - 1, W, E, 0), b"overlap"), ((img.data_ptr(), img.data_ptr(), good, H, W, E, 0), b"overlap")]
        before = img.clone()
        for args, word in dev_cases:
            lib.stm_d_rectify(*args)
            msg = lib.stm_last_error()
            torch.cuda.synchronize()
            assert b"d_rectify" in msg and word in msg, (args[3:], msg)
            assert (out == FILL).all() and torch.equal(img, before), args[3:]
        host_cases = [((None, u8(h_img), good, H, W, E, 0), b"null"), ((u8(h_out), u8(h_img), None, H, W, E, 0), b"null"),
                      ((u8(h_out), u8(h_img), good, H, 16385, E, 0), b"num_cols"), ((u8(h_out), u8(h_img), good, H, W, 1, 0), b"elem_sz"),
                      ((u8(h_out), u8(h_img), good, H, W, E, 7), b"border"), ((u8(h_out), u8(h_img), recs["nan"][1], H, W, E, 0), b"finite"),
                      ((u8(h_img), u8(h_img), good, H, W, E, 0), b"overlap")]
        for args, word in host_cases:
            lib.stm_rectify(*args)
            msg = lib.stm_last_error()
            assert b"rectify" in msg and b"d_rectify" not in msg and word in msg, (args[3:], msg)
            assert (h_out == FILL).all() and np.array_equal(h_img, texture(H, W, 1)), args[3:]
        for args, word in [((None, good, H, W), b"null"), ((ip, None, H, W), b"null"), ((ip, good, 0, W), b"num_rows"), ((ip, good, H, 16385), b"num_cols"),
                           ((ip, recs["inf"][1], H, W), b"finite")]:
            lib.stm_rectify_coords(*args)
            msg = lib.stm_last_error()
            assert b"rectify_coords" in msg and word in msg, msg
            assert (quv == 5).all()
    finally:
        lib.stm_set_error_mode(0)
    lib.stm_d_rectify(out.data_ptr(), img.data_ptr(), good, H, W, E, 0)  # and the same buffers are served once the arguments are right
    torch.cuda.synchronize()
    assert torch.equal(out, img)


# ------------------------------------------------------------------------------------------------------- 2. the frame
N_FRAMES = 7  # per slot: an eager frame, the capture, a replay
_PAIRS = {}


def _params():
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=ZD, usd=17, lsd=8)


def _pair(H, W, k):
    """frame k of a small sequence: one synthetic stereo pair under fresh noise of +-2 per channel (the colour gate of the temporal
    step stays open), black bars of 3 rows (the active area has something to find)"""
    from stm_amd import synth
    if (H, W, k) not in _PAIRS:
        L, R, _ = synth.stereo_pair(H, W, D, ZD, seed=77)
        rng = np.random.RandomState(k)
        pair = []
        for a in (L, R):
            a = np.clip(a.astype(np.int32) + rng.randint(-2, 3, size=a.shape), 0, 255).astype(np.uint8)
            a[:3] = 0
            a[-3:] = 0
            a.setflags(write=False)
            pair.append(a)
        _PAIRS[(H, W, k)] = tuple(pair)
    return _PAIRS[(H, W, k)]


def _records(H, W):
    """a camera pair that is nearly rectified: the left eye rolled by half a degree under a little barrel, the right eye rolled the
    other way, a focal ratio of 1.01 and a principal point off the centre"""
    from stm_amd import rectify
    cx, cy, f = (W - 1) / 2.0, (H - 1) / 2.0, 1.1 * W
    rec_l = rectify.record(camera(f, cx, cy), [-0.08, 0.01, 1e-3, -5e-4, 0.0], rot_z(0.5), camera(f, cx, cy))
    rec_r = rectify.record(camera(f, cx + 0.7, cy - 0.4, 1.01), [0.05, 0.0, 0.0, 0.0, 0.0], rot_z(-0.4), camera(f, cx, cy))
    return rec_l, rec_r


def _inputs(fmt, L, R):
    """(the stream's keywords, the frame as the stream takes it, the unpacked eyes as the statement sees them)"""
    from stm_amd import synth
    H, W = L.shape[:2]
    if fmt == "bgr":
        return {}, np.ascontiguousarray(np.concatenate([L, R], axis=1)), (L, R)
    if fmt == "nv12":
        y, uv = synth.bgr_to_nv12(np.concatenate([L, R], axis=1), 0)
        return dict(input_format="nv12"), nv12_frame(y, uv), unpack_nv12_ref(y, uv, H, W, (0, 0, 0), 0, 0)
    assert fmt == "half"  # half-width side by side, the right eye first, Catmull-Rom, a gap of 2: 67 x 130 comes 132 wide
    f = synth.pack_frame(L, R, 1, 1, 2, fill=0x33)
    return dict(packing=(1, 1, 1, 2)), f, unpack_ref(f, H, W, (1, 1, 1), 2)


def _stream(frames, H, W, **kw):
    from stm_amd import video
    fs = video.FrameStream(H, W, _params(), **kw)
    outs = []
    try:
        pending = 0
        for f in frames:
            if pending == 2:
                outs.append(fs.collect())
                pending -= 1
            fs.submit(f)
            pending += 1
        while pending:
            outs.append(fs.collect())
            pending -= 1
    finally:
        fs.close()
    return outs


EXTRAS = dict(align_auto=(5, 0.5), cut=True, active_auto=True)
CASES = [("bgr", 48, 96, 3, {}), ("bgr", 67, 130, 3 | T, {}), ("nv12", 48, 96, 3, {}), ("nv12", 48, 96, 3 | T, {}), ("half", 67, 130, 3, {}),
         ("half", 48, 96, 3 | T, {}), ("bgr", 48, 96, 3, EXTRAS), ("bgr", 67, 130, 3 | T, EXTRAS), ("nv12", 48, 96, 3, EXTRAS), ("half", 48, 96, 3 | T, EXTRAS),
         ("bgr", 48, 96, 3, dict(match=(24, 48, 0.5))), ("nv12", 48, 96, 3 | T, dict(match=(24, 48, 0.5))), ("bgr", 67, 130, 3, dict(match=(33, 65, 0.5)))]


@pytest.mark.parametrize("border", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s_%dx%d_%x_%s" % (c[0], c[1], c[2], c[3], "+".join(sorted(c[4])) or "plain"))
def test_stream_with_rectification_is_the_stream_on_the_rectified_frames(gpu_ready, case, border):
    """seven frames: the frame and both maps of a stream with the setting on the raw frames are those of the same stream without it
    on the statement's rectified frames, whatever the input format, the packing, the stages and the settings behind it.  One
    combination has no BGR stream to be compared with and is not here: NV12 input with 0x2000 AND an alignment (or a balance) -- an
    NV12 stream's history is the other slot's split images as that frame aligned them, a BGR stream's the previous frame put through
    the current frame's field (DESIGN.md sections 23 and 32); NV12 with 0x2000 alone, and NV12 with the alignment alone, are."""
    fmt, H, W, stages, extra = case
    rec_l, rec_r = _records(H, W)
    raw, rect = [], []
    for k in range(N_FRAMES):
        kw, frame, (eye_l, eye_r) = _inputs(fmt, *_pair(H, W, k))
        raw.append(frame)
        rect.append(np.ascontiguousarray(np.concatenate([rectify_ref(eye_l, rec_l, border), rectify_ref(eye_r, rec_r, border)], axis=1)))
    assert not np.array_equal(rect[0][:, :W], _inputs(fmt, *_pair(H, W, 0))[2][0])
    got = _stream(raw, H, W, stages=stages, rectify=(rec_l, rec_r, border), **kw, **extra)
    want = _stream(rect, H, W, stages=stages, **extra)
    assert len(got) == len(want) == N_FRAMES
    for k in range(N_FRAMES):
        assert got[k][0] == want[k][0] == k
        for j in range(1, 4):
            assert np.array_equal(got[k][j], want[k][j]), (case[:4], border, k, j)
        assert want[k][1].any() and want[k][3].any()
    if "active_auto" in extra:  # the bars were found on the rectified frame
        assert 0 < np.count_nonzero(want[-1][3])


def test_stream_entry_rules(gpu_ready, lib):
    from stm_amd import video
    H, W = 48, 96
    rec_l, rec_r = _records(H, W)
    rec = np.ascontiguousarray(np.stack([rec_l, rec_r]))
    bad = rec.copy()
    bad[1, 4] = np.nan
    p = lambda a: a.ctypes.data_as(f32p)
    frame = np.ascontiguousarray(np.concatenate(_pair(H, W, 0), axis=1))
    lib.stm_set_error_mode(1)
    try:
        fs = video.FrameStream(H, W, _params())
        try:
            assert fs.get_rectify() is None
            for args, word in [((2, p(rec), 0), b"mode"), ((-1, p(rec), 0), b"mode"), ((1, None, 0), b"null"), ((1, p(rec), 2), b"border"),
                               ((1, p(bad), 0), b"finite")]:
                assert lib.stm_stream_rectify(fs._h, *args) == -1
                msg = lib.stm_last_error()
                assert b"stream_rectify" in msg and word in msg, msg
                assert fs.get_rectify() is None
            assert lib.stm_stream_rectify(fs._h, 1, p(rec), 1) == 0
            got = fs.get_rectify()
            assert np.array_equal(got[0], rec_l) and np.array_equal(got[1], rec_r) and got[2] == 1
            assert lib.stm_stream_input_depth(fs._h, 2, 12.0, -12.0, 0, 0.0) == -1  # the mirrored refusal
            msg = lib.stm_last_error()
            assert b"stream_input_depth" in msg and b"rectif" in msg, msg
            assert lib.stm_stream_rectify(fs._h, 0, None, 0) == 0 and fs.get_rectify() is None
            assert lib.stm_stream_rectify(fs._h, 1, p(rec), 0) == 0
            assert fs.submit(frame) == 0
            for args in ((0, None, 0), (1, p(rec), 1)):  # only before the first submit
                assert lib.stm_stream_rectify(fs._h, *args) == -1
                assert b"stream_rectify" in lib.stm_last_error()
            assert fs.get_rectify()[2] == 0
            fs.collect()
        finally:
            fs.close()
        fs = video.FrameStream(H, W, _params(), depth_input=("u8", 12.0, -12.0))
        try:
            assert lib.stm_stream_rectify(fs._h, 1, p(rec), 0) == -1
            msg = lib.stm_last_error()
            assert b"stream_rectify" in msg and b"depth input" in msg, msg
            assert lib.stm_stream_rectify(fs._h, 0, None, 0) == 0  # off stays possible
        finally:
            fs.close()
        with pytest.raises(ValueError):
            video.FrameStream(H, W, _params(), depth_input=("u8", 12.0, -12.0), rectify=(rec_l, rec_r))
        q = _params()
        h = lib.stm_stream_create(H, 2 * W - 1, W, H, W, 3, q.num_views, q.angle, q.num_disp, q.zero_disp, q.ad_coeff, q.census_coeff, q.ucd, q.lcd,
                                  q.usd, q.lsd, q.thresh_s, q.thresh_h)
        try:
            assert lib.stm_stream_rectify(h, 1, p(rec), 0) == -1  # a BGR frame too narrow to hold both eyes
            msg = lib.stm_last_error()
            assert b"stream_rectify" in msg and b"num_cols_sbs" in msg, msg
        finally:
            lib.stm_stream_destroy(h)
    finally:
        lib.stm_set_error_mode(0)


_FRESH = """
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from test_gpu_rectify import _pair, _stream
H, W = 48, 96
frames = [np.ascontiguousarray(np.concatenate(_pair(H, W, k), axis=1)) for k in range(3)]
h = hashlib.sha256()
for out in _stream(frames, H, W):
    for a in out[1:]:
        h.update(np.ascontiguousarray(a).tobytes())
print("digest", h.hexdigest())
"""


def test_a_stream_without_the_entry_is_what_a_fresh_process_computes(gpu_ready):
    """after every stream above: a stream that never called stm_stream_rectify gives the bytes of a process that never saw one"""
    H, W = 48, 96
    rec_l, rec_r = _records(H, W)
    frames = [np.ascontiguousarray(np.concatenate(_pair(H, W, k), axis=1)) for k in range(3)]
    _stream(frames, H, W, rectify=(rec_l, rec_r, 1))  # this thread has just run rectified frames
    h = hashlib.sha256()
    for out in _stream(frames, H, W):
        for a in out[1:]:
            h.update(np.ascontiguousarray(a).tobytes())
    text = subprocess.check_output([sys.executable, "-c", _FRESH % (ROOT, os.path.join(ROOT, "tests"))], cwd=ROOT).decode()
    assert "digest " + h.hexdigest() in text


# ------------------------------------------------------------------------------------------------------- 3. the two drivers
def test_video_and_image_cli_with_rectification(gpu_ready, tmp_path):
    """tools/stm_video.py --rectify FILE 1 on a directory of BMP frames writes the per-frame calls' frames on the statement's rectified
    pairs; tools/stm_image.py --rectify FILE hands the rectified images to its chain (view 0 is the right image, the last the left)"""
    import torch
    from stm_amd import bmp_io, device_api as dev
    H, W, n = 48, 96, 3
    rec_l, rec_r = _records(H, W)
    np.save(str(tmp_path / "rec.npy"), np.stack([rec_l, rec_r]))
    pairs = [_pair(H, W, k) for k in range(n)]
    src = tmp_path / "in"
    src.mkdir()
    for k, pr in enumerate(pairs):
        bmp_io.write_bmp(str(src / ("f_%03d.bmp" % k)), np.ascontiguousarray(np.concatenate(pr, axis=1)))
    out = tmp_path / "o"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "stm_video.py"), str(src), "8", "18.43", str(W), str(H), str(D), str(ZD),
                           "10", "30", "6", "20", "17", "8", "20", "0.4", str(out), "--rectify", str(tmp_path / "rec.npy"), "1"],
                          stdout=subprocess.DEVNULL)
    p = dev.FrameParams(num_disp=D, zero_disp=ZD, usd=17, lsd=8, angle=18.0)  # the tool truncates the slant
    for k, (L, R) in enumerate(pairs):
        rect = np.ascontiguousarray(np.concatenate([rectify_ref(L, rec_l, 1), rectify_ref(R, rec_r, 1)], axis=1))
        dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        dr, o = torch.zeros_like(dl), torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        dev.d_adcensus_stm(torch.from_numpy(rect).cuda(), dl, dr, o, p, stages=3)
        assert np.array_equal(bmp_io.read_bmp(str(out / ("interlaced_%05d.bmp" % k))), o.cpu().numpy()), k
    L, R = pairs[0]
    bmp_io.write_bmp(str(tmp_path / "l.bmp"), L)
    bmp_io.write_bmp(str(tmp_path / "r.bmp"), R)
    img_out = tmp_path / "i"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "stm_image.py"), str(tmp_path / "l.bmp"), str(tmp_path / "r.bmp"), "10", "30",
                           str(D), str(ZD), "6", "20", "17", "8", "8", "18.43", str(W), str(H), "20", "0.4", str(img_out), "--rectify",
                           str(tmp_path / "rec.npy")], stdout=subprocess.DEVNULL)
    assert np.array_equal(bmp_io.read_bmp(str(img_out / "view_0.bmp")), rectify_ref(R, rec_r, 0))
    assert np.array_equal(bmp_io.read_bmp(str(img_out / "view_7.bmp")), rectify_ref(L, rec_l, 0))
