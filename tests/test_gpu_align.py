"""The vertical alignment on the GPU (stm_set_align, stm_align_rows, stm_align_fit, the frame calls and the frame stream), bit for
bit against the numpy statement in tests/test_align_ref.py.  The frame calls' oracle is the same call with alignment off on the
statement's aligned frame."""
import ctypes as C

import numpy as np
import pytest

from test_align_ref import (KB, KR, align_frame_ref, align_rows_ref, displace, field_q, measure_ref, _texture)
from test_packing_ref import unpack_nv12_ref, unpack_ref

pytestmark = pytest.mark.gpu

T = 0x2000
FILL = 0x77
D, ZD = 16, 8


@pytest.fixture(autouse=True)
def _alignment_off_afterwards(gpu_ready):
    from stm_amd import device_api as dev
    assert dev.get_align()[0] == 0
    yield
    assert dev.get_align()[0] == 0, "a test left the thread's alignment on"
    assert dev.get_packing() == dev.PACKING_OFF


@pytest.fixture
def lib(stm, gpu_ready):
    import torch
    l = stm.lib()
    l.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return l


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


# ------------------------------------------------------------------------------------------------------- 1. the stage: apply
WIDTHS = [1, 2, 3, 17, 63, 64, 65, 130, 257, 300]
ROWS = [1, 2, 3, 4, 5, 33]


def _fields(H, W):
    """(a, b, c) and what each is there for; the checks below prove each does what its name says on this shape"""
    return [("multiple of 16", (2.0, 0.0, 0.0)), ("negative multiple", (-1.0, 0.0, 0.0)), ("f = 15", (15.0 / 16.0, 0.0, 0.0)),
            ("f = 15 below zero", (-1.0 / 16.0, 0.0, 0.0)), ("both taps clamp", (float(H + 7), 0.0, 0.0)),
            ("both taps clamp at the top", (-float(H + 7), 0.0, 0.0)), ("clamp +64", (100.0, 0.0, 0.0)), ("clamp -64", (-100.0, 0.0, 0.0)),
            ("tilt across the width", (0.3, 0.06, 0.0)), ("tilt down the height", (-0.2, 0.0, 0.35)), ("all three", (1.7, -0.05, 0.21))]


def test_fields_do_what_their_names_say():
    q = field_q(33, 130, 2.0, 0.0, 0.0)
    assert (q == 32).all()
    assert (field_q(5, 3, 15.0 / 16.0, 0, 0) == 15).all() and (field_q(5, 3, -1.0 / 16.0, 0, 0) == -1).all()
    assert (field_q(5, 3, 12.0, 0, 0) >> 4 >= 5).all()
    assert (field_q(80, 17, 100.0, 0, 0) == 1024).all() and (field_q(80, 17, -100.0, 0, 0) == -1024).all()
    q = field_q(33, 130, 0.3, 0.06, 0.0)
    for x0 in (0, 64):  # the whole-row part changes inside each wave of 64 columns
        assert len(set((q[0, x0:x0 + 64] >> 4).tolist())) > 1
    assert len(set((field_q(33, 5, -0.2, 0.0, 0.35)[:, 0] >> 4).tolist())) > 1


@pytest.mark.parametrize("E", [3, 4])
def test_align_rows_device(lib, E):
    """every width x every row count x every field, caller buffers at byte offsets 0 .. 3 (input and output differently), the
    bytes past a pixel's third left alone, nothing outside the output written; 80 x 17 distinguishes the clamp at 64 rows from
    none"""
    from test_gpu_caller_buffers import Arena, P, read
    n = 0
    for W in WIDTHS:
        arena = Arena(True, nbytes=12 << 20)
        cases = []
        for H in ROWS + ([80] if W == 17 else []):
            img = np.full((H, W, E), 0xC3, np.uint8)
            img[:, :, :3] = _texture(H, W, H * 1000 + W)
            d_img = arena.put(img, n % 4)
            for name, (a, b, c) in _fields(H, W):
                d_out = arena.put(np.full((H, W, E), FILL, np.uint8), (n // 4 + n) % 4)
                lib.stm_d_align_rows(P(d_out), P(d_img), H, W, E, a, b, c)
                cases.append((name, H, (a, b, c), img, d_out))
                n += 1
        assert arena.intact(), W
        for name, H, f, img, d_out in cases:
            got = read(d_out, np.uint8, (H, W, E))
            assert np.array_equal(got[:, :, :3], align_rows_ref(img, *f)), (name, H, W, E)
            assert (got[:, :, 3:] == FILL).all(), (name, H, W, E)
    big = _texture(80, 17, 5)  # the clamp at 64 rows is seen: an unclamped shift by 100 rows would repeat the last row everywhere
    assert not np.array_equal(align_rows_ref(big, 100.0, 0, 0), big[np.clip(np.arange(80) + 100, 0, 79)])
    assert np.array_equal(align_rows_ref(big, 100.0, 0, 0), big[np.clip(np.arange(80) + 64, 0, 79)])


def test_align_rows_host(gpu_ready):
    from stm_amd import host_api as api
    for (H, W, E) in [(5, 65, 3), (33, 130, 4)]:
        img = np.full((H, W, E), 0xC3, np.uint8)
        img[:, :, :3] = _texture(H, W, 9)
        for name, f in _fields(H, W):
            got = api.align_rows(img, *f)
            assert np.array_equal(got[:, :, :3], align_rows_ref(img, *f)) and (got[:, :, 3:] == 0).all(), (name, H, W, E)
        assert np.array_equal(api.align_rows(img, 0.0, 0.0, 0.0)[:, :, :3], img[:, :, :3])


# ------------------------------------------------------------------------------------------------------- 2. the measurement
SHAPES = [(4, 8), (40, 64), (67, 130), (97, 300)]
_MEASURE = {}


def _measure_inputs(H, W):
    """name -> (left, right): textured pairs displaced by known fields, a flat pair, and texture in one band only"""
    if (H, W) not in _MEASURE:
        tex = _texture(H, W, H + W)
        flat = np.full((H, W, 3), 131, np.uint8)
        one = flat.copy()
        x0, x1 = 5 * W // KB, 6 * W // KB
        one[:, x0:x1] = tex[:, x0:x1]
        pairs = {"shift": (tex, displace(tex, min(2.25, H / 8.0), 0.0, 0.0)),
                 "plane": (tex, displace(tex, -0.6, 0.9 / W, 1.3 / H)),
                 "flat": (flat, flat.copy()),
                 "one band": (one, displace(one, 1.0, 0.0, 0.0))}
        for pair in pairs.values():
            for a in pair:
                a.setflags(write=False)
        _MEASURE[(H, W)] = pairs
    return _MEASURE[(H, W)]


@pytest.mark.parametrize("R", [1, 5, 32])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_align_fit_device(gpu_ready, shape, R):
    """profiles and SADs as integers, the state as bit patterns, the number of valid blocks; 3- and 4-byte pixels"""
    import torch
    from stm_amd import device_api as dev
    H, W = shape
    seen_valid = False
    for k, (name, (left, right)) in enumerate(sorted(_measure_inputs(H, W).items())):
        E = 3 + k % 2
        imgs = []
        for v in (left, right):
            a = np.full((H, W, E), 0x3C, np.uint8)
            a[:, :, :3] = v
            imgs.append(_cuda(a))
        state = torch.zeros(4, dtype=torch.float32, device="cuda")
        nv = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        prof = torch.full((2 * KB * H,), -1, dtype=torch.int32, device="cuda")
        sad = torch.full((KB * KR * (2 * R + 1),), -1, dtype=torch.int32, device="cuda")
        dev.d_align_fit(imgs[0], imgs[1], R, 1.0, state, nv, prof, sad)
        torch.cuda.synchronize()
        P, S, want, nvalid = measure_ref(left, right, R, state=np.zeros(4, np.float32))
        assert np.array_equal(prof.cpu().numpy().view(np.uint32).reshape(2, KB, H), P), (name, "profiles")
        assert np.array_equal(sad.cpu().numpy().view(np.uint32).reshape(KB, KR, 2 * R + 1), S), (name, "S")
        assert int(nv.item()) == nvalid, name
        assert _bits(state.cpu().numpy()) == _bits(want), (name, state.cpu().numpy(), want)
        seen_valid |= nvalid > 0
        if name == "flat":
            assert nvalid == 0 and not state.cpu().numpy().any()
    assert seen_valid or (H, W) == (4, 8)


def test_align_fit_recursive_update_and_host_flavour(gpu_ready):
    """four frames through one state at rate 0.25 (the third without a valid block: the state is kept), device and host flavour"""
    import torch
    from stm_amd import device_api as dev, host_api as api
    H, W, R = 67, 130, 5
    pairs = _measure_inputs(H, W)
    seq = [pairs["shift"], pairs["plane"], pairs["flat"], pairs["one band"]]
    state = torch.zeros(4, dtype=torch.float32, device="cuda")
    want = np.zeros(4, np.float32)
    host = np.zeros(4, np.float32)
    for left, right in seq:
        dev.d_align_fit(_cuda(left), _cuda(right), R, 0.25, state)
        torch.cuda.synchronize()
        _, _, want, nvalid = measure_ref(left, right, R, state=want, rate=0.25)
        assert _bits(state.cpu().numpy()) == _bits(want)
        host, n = api.align_fit(left, right, R, 0.25, host)
        assert _bits(host) == _bits(want) and n == nvalid
    assert want[0] == 1.0 and want[1] != 0.0


# ------------------------------------------------------------------------------------------------------- 3. the frame calls
_PAIRS = {}
FIELD = (2.6, 0.011, -0.017)


def _pair(H, W, k=0):
    """frame k of a small sequence: one synthetic stereo pair under fresh noise of +-2 per channel (the colour gate of the temporal
    step stays open), its right eye displaced vertically, a little further in every frame"""
    from stm_amd import synth
    if (H, W, k) not in _PAIRS:
        L, R, _ = synth.stereo_pair(H, W, D, ZD, seed=77)
        rng = np.random.RandomState(k)
        L = np.clip(L.astype(np.int32) + rng.randint(-2, 3, size=L.shape), 0, 255).astype(np.uint8)
        R = np.clip(R.astype(np.int32) + rng.randint(-2, 3, size=R.shape), 0, 255).astype(np.uint8)
        R = displace(R, FIELD[0] + 0.3 * k, FIELD[1], FIELD[2])
        L.setflags(write=False)
        R.setflags(write=False)
        _PAIRS[(H, W, k)] = (L, R)
    return _PAIRS[(H, W, k)]


def _params():
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=ZD, usd=17, lsd=8)


def _outputs(H, W):
    import torch
    dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    return dl, torch.zeros_like(dl), torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")


def _frame_call(kind, inp, H, W, stages, hist=None, reduced=None):
    """one frame call with the thread's settings as they are.  kind "bgr": inp a side-by-side or packed BGR frame, "nv12": (y, uv).
    hist = (previous frame, prev dl, prev dr) for 0x2000 through _t; reduced = (h, w, scale): the _2s call.  Returns numpy outputs."""
    import torch
    from stm_amd import device_api as dev
    p = _params()
    dl, dr, out = _outputs(H, W)
    if kind == "nv12":
        il = torch.full((H, W, 3), FILL, dtype=torch.uint8, device="cuda")
        ir = torch.full_like(il, FILL)
        dev.d_adcensus_stm_nv12(_cuda(inp[0]), _cuda(inp[1]), dl, dr, out, p, stages, 0, il, ir)
        torch.cuda.synchronize()
        return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy(), il.cpu().numpy(), ir.cpu().numpy()
    d_in = _cuda(inp)
    if reduced is not None:
        dev.d_adcensus_stm_2s(d_in, dl, dr, out, p, reduced[0], reduced[1], reduced[2], stages)
    elif stages & T:
        h = [None] * 3 if hist is None else [_cuda(a) for a in hist]
        dev.d_adcensus_stm_t(d_in, dl, dr, out, p, stages, h[0], h[1], h[2])
    else:
        dev.d_adcensus_stm(d_in, dl, dr, out, p, stages=stages)
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), inp)  # read only
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


class _Aligned:
    """the thread's alignment for the duration of a block; mode 2 with a device state or None"""

    def __init__(self, mode, field=(0.0, 0.0, 0.0), radius=5, rate=1.0, state=None):
        self.args = (mode, field, radius, rate, state)

    def __enter__(self):
        from stm_amd import device_api as dev
        mode, field, radius, rate, state = self.args
        if mode == 2:
            dev.set_align_auto(radius, rate, state)
        dev.set_align(mode, *field)

    def __exit__(self, *exc):
        from stm_amd import device_api as dev
        dev.set_align_auto(16, 1.0, None)
        dev.set_align(0)


def _same(got, want, what):
    for k in range(3):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert want[0].any() and want[2].any(), what


def _inputs(fmt, L, R):
    """(kind, the call's input, packing, the unpacked eyes as the statement sees them)"""
    from stm_amd import synth
    H, W = L.shape[:2]
    if fmt == "bgr":
        return "bgr", np.ascontiguousarray(np.concatenate([L, R], axis=1)), None, (L, R)
    if fmt == "nv12":
        y, uv = synth.bgr_to_nv12(np.concatenate([L, R], axis=1), 0)
        return "nv12", (y, uv), None, unpack_nv12_ref(y, uv, H, W, (0, 0, 0), 0, 0)
    assert fmt == "half"  # half-width side by side, the right eye first, Catmull-Rom, a gap of 6
    f = synth.pack_frame(L, R, 1, 1, 6, fill=0x33)
    return "bgr", f, (1, 1, 1, 6), unpack_ref(f, H, W, (1, 1, 1), 6)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case", [("bgr", 48, 96), ("bgr", 67, 130), ("nv12", 48, 96), ("half", 48, 96), ("half", 67, 132)],
                         ids=lambda c: "%s_%dx%d" % c)
def test_frame_under_alignment_is_the_plain_frame_on_the_aligned_pair(gpu_ready, case, mode):
    """stm_d_adcensus_stm / _nv12 at stages 3 and 3 | 0x200 | 0x400 | 0x800, and _2s (BGR); mode 2 with a null state"""
    from stm_amd import device_api as dev
    fmt, H, W = case
    kind, inp, pk, (eye_l, eye_r) = _inputs(fmt, *_pair(H, W))
    if mode == 1:
        field = FIELD
    else:
        _, _, st, nvalid = measure_ref(eye_l, eye_r, 5)
        assert st[0] == 1.0 and nvalid >= 3 and abs(st[1]) > 1.0  # the measurement found the displacement
        field = tuple(float(v) for v in st[1:])
    aligned = np.ascontiguousarray(align_frame_ref(eye_l, eye_r, *field))
    assert not np.array_equal(aligned[:, W:], eye_r)
    before = _frame_call(kind, inp, H, W, 3) if pk is None else None
    for stages in (3, 3 | 0x200 | 0x400 | 0x800):
        want = _frame_call("bgr", aligned, H, W, stages)
        if pk is not None:
            dev.set_packing(*pk)
        try:
            with _Aligned(mode, FIELD):
                got = _frame_call(kind, inp, H, W, stages)
        finally:
            dev.set_packing(0, 0, 0, 0)
        _same(got, want, (case, mode, stages))
        if kind == "nv12":  # the split images the call hands out are the aligned eyes
            assert np.array_equal(got[3], aligned[:, :W]) and np.array_equal(got[4], aligned[:, W:])
    if fmt == "bgr":
        red = (H // 2, W // 2, 0.5)
        want = _frame_call("bgr", aligned, H, W, 3, reduced=red)
        with _Aligned(mode, FIELD):
            got = _frame_call("bgr", inp, H, W, 3, reduced=red)
        _same(got, want, (case, mode, "_2s"))
    if pk is None:  # off again: the bytes of the call before any alignment was set, which are not the aligned frame's
        after = _frame_call(kind, inp, H, W, 3)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        assert not np.array_equal(after[0], _frame_call("bgr", aligned, H, W, 3)[0])


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("fmt", ["bgr", "half"])
def test_temporal_history_goes_through_the_current_field(gpu_ready, fmt, mode):
    """0x2000 through _t: the previous frame is aligned with the CURRENT frame's field; mode 2 with a device state carried over
    from the previous frame at rate 0.5, so the current field differs from what either frame alone would give"""
    import torch
    from stm_amd import device_api as dev
    H, W = 48, 96
    (kind, prev_in, pk, prev_eyes), (_, cur_in, _, cur_eyes) = _inputs(fmt, *_pair(H, W, 0)), _inputs(fmt, *_pair(H, W, 1))
    if mode == 1:
        field, state = FIELD, None
    else:
        _, _, st0, _ = measure_ref(prev_eyes[0], prev_eyes[1], 5, state=np.zeros(4, np.float32))
        _, _, st1, _ = measure_ref(cur_eyes[0], cur_eyes[1], 5, state=st0, rate=0.5)
        assert st0[0] == 1.0 and _bits(st0) != _bits(st1)
        field, state = tuple(float(v) for v in st1[1:]), _cuda(st0)
    cur_al = np.ascontiguousarray(align_frame_ref(cur_eyes[0], cur_eyes[1], *field))
    prev_al = np.ascontiguousarray(align_frame_ref(prev_eyes[0], prev_eyes[1], *field))
    first = _frame_call("bgr", prev_al, H, W, 2)
    ql, qr = first[0] + np.float32(0.25), first[1] - np.float32(0.25)
    want = _frame_call("bgr", cur_al, H, W, 2 | T, (prev_al, ql, qr))
    assert not np.array_equal(want[0], _frame_call("bgr", cur_al, H, W, 2)[0])  # the step did something
    if pk is not None:
        dev.set_packing(*pk)
    try:
        with _Aligned(mode, FIELD, rate=0.5, state=state):
            got = _frame_call(kind, cur_in, H, W, 2 | T, (prev_in, ql, qr))
    finally:
        dev.set_packing(0, 0, 0, 0)
    for k in range(2):
        assert np.array_equal(got[k], want[k]), (fmt, mode, k)
    if mode == 2:
        torch.cuda.synchronize()
        assert _bits(state.cpu().numpy()) == _bits(st1)


def test_frame_rules(gpu_ready, lib):
    """a frame too narrow to hold both eyes, and a frame too small for the measurement, are refused with nothing written"""
    import torch
    from stm_amd import device_api as dev
    lib.stm_set_error_mode(1)
    try:
        p = _params()
        for (mode, H, W, Wsbs, word) in [(1, 8, 16, 24, b"num_cols_sbs"), (2, 3, 16, 32, b"num_rows"), (2, 8, 6, 12, b"num_cols")]:
            sbs = torch.zeros((H, Wsbs, 3), dtype=torch.uint8, device="cuda")
            dl = torch.full((H, W), 5.0, dtype=torch.float32, device="cuda")
            dr, out = torch.full_like(dl, 5.0), torch.full((H, W, 3), FILL, dtype=torch.uint8, device="cuda")
            with _Aligned(mode, FIELD):
                lib.stm_d_adcensus_stm(sbs.data_ptr(), dl.data_ptr(), dr.data_ptr(), out.data_ptr(), H, Wsbs, W, H, W, 3, p.num_views, p.angle,
                                       p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, 3)
            msg = lib.stm_last_error()
            torch.cuda.synchronize()
            assert b"d_adcensus_stm" in msg and word in msg, msg
            assert (dl == 5.0).all() and (out == FILL).all()
    finally:
        lib.stm_set_error_mode(0)


# ------------------------------------------------------------------------------------------------------- 4. the frame stream
def _stream(frames, H, W, **kw):
    from stm_amd import video
    fs = video.FrameStream(H, W, _params(), **kw)
    outs, fields = [], []
    try:
        pending = 0
        for f in frames:
            if pending == 2:
                outs.append(fs.collect())
                fields.append(fs.align())
                pending -= 1
            fs.submit(f)
            pending += 1
        while pending:
            outs.append(fs.collect())
            fields.append(fs.align())
            pending -= 1
    finally:
        fs.close()
    return outs, fields


@pytest.mark.parametrize("mode", [1, 2])
def test_stream_under_alignment(gpu_ready, mode):
    """six frames, so that both slots' captured graphs replay: every frame is the plain frame call on the statement's aligned frame,
    and stm_stream_align reports the statement's state (mode 2: carried from frame to frame at rate 0.5)"""
    from stm_amd import device_api as dev
    H, W, n = 48, 96, 6
    pairs = [_pair(H, W, k) for k in range(n)]
    frames = [np.ascontiguousarray(np.concatenate(pr, axis=1)) for pr in pairs]
    dev.set_align(1, 9.0, 0.0, 0.0)  # the calling thread's own setting never reaches a stream's frames
    try:
        if mode == 1:
            outs, fields = _stream(frames, H, W, align=FIELD)
        else:
            outs, fields = _stream(frames, H, W, align_auto=(5, 0.5))
        plain, _ = _stream(frames[:2], H, W)
    finally:
        dev.set_align(0)
    st = np.zeros(4, np.float32)
    for k in range(n):
        if mode == 1:
            field = FIELD
            assert _bits(fields[k]) == _bits(FIELD)
        else:
            _, _, st, _ = measure_ref(pairs[k][0], pairs[k][1], 5, state=st, rate=0.5)
            field = tuple(float(v) for v in st[1:])
            assert _bits(fields[k]) == _bits(st[1:]), (k, fields[k], st)
        want = _frame_call("bgr", np.ascontiguousarray(align_frame_ref(pairs[k][0], pairs[k][1], *field)), H, W, 3)
        assert outs[k][0] == k
        for j in range(3):
            assert np.array_equal(outs[k][1 + j], want[j]), (mode, k, j)
    for k in range(2):  # a stream without the setting: today's bytes, whatever the thread has set
        want = _frame_call("bgr", frames[k], H, W, 3)
        for j in range(3):
            assert np.array_equal(plain[k][1 + j], want[j]), ("off", k, j)


# ------------------------------------------------------------------------------------------------------- 5. the two drivers
def test_video_and_image_cli_with_alignment(gpu_ready, tmp_path):
    """tools/stm_video.py --align-auto RADIUS RATE on a directory of BMP frames writes the per-frame calls' frames on the statement's
    aligned pairs and prints each frame's field; tools/stm_image.py --align-auto RADIUS hands the aligned right image to its chain
    (view 0 is the right image); malformed options are refused"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from stm_amd import bmp_io
    H, W, n = 48, 96, 3
    pairs = [_pair(H, W, k) for k in range(n)]
    src = tmp_path / "in"
    src.mkdir()
    for k, pr in enumerate(pairs):
        bmp_io.write_bmp(str(src / ("f_%03d.bmp" % k)), np.ascontiguousarray(np.concatenate(pr, axis=1)))
    out = tmp_path / "o"
    args = [sys.executable, os.path.join(ROOT, "tools", "stm_video.py"), str(src), "8", "18.43", str(W), str(H), str(D), str(ZD),
            "10", "30", "6", "20", "17", "8", "20", "0.4", str(out)]
    text = subprocess.check_output(args + ["--align-auto", "5", "0.5"]).decode()
    st = np.zeros(4, np.float32)
    for k in range(n):
        _, _, st, _ = measure_ref(pairs[k][0], pairs[k][1], 5, state=st, rate=0.5)
        assert "frame %d: align a %.6g b %.6g c %.6g" % ((k,) + tuple(float(v) for v in st[1:])) in text, (k, text)
        aligned = np.ascontiguousarray(align_frame_ref(pairs[k][0], pairs[k][1], *[float(v) for v in st[1:]]))
        from stm_amd import device_api as dev
        p = dev.FrameParams(num_disp=D, zero_disp=ZD, usd=17, lsd=8, angle=18.0)  # the tool truncates the slant
        dl, dr, o = _outputs(H, W)
        dev.d_adcensus_stm(_cuda(aligned), dl, dr, o, p, stages=3)
        assert np.array_equal(bmp_io.read_bmp(str(out / ("interlaced_%05d.bmp" % k))), o.cpu().numpy()), k
    for bad in (["--align", "1", "2"], ["--align-auto", "40"], ["--align-auto", "5", "1.5"], ["--align", "1", "0", "0", "--align-auto", "5"]):
        assert subprocess.call(args + bad, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0, bad
    L, R = pairs[0]
    bmp_io.write_bmp(str(tmp_path / "l.bmp"), L)
    bmp_io.write_bmp(str(tmp_path / "r.bmp"), R)
    img_out = tmp_path / "i"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "stm_image.py"), str(tmp_path / "l.bmp"), str(tmp_path / "r.bmp"), "10", "30",
                           str(D), str(ZD), "6", "20", "17", "8", "8", "18.43", str(W), str(H), "20", "0.4", str(img_out), "--align-auto", "5"],
                          stdout=subprocess.DEVNULL)
    _, _, st0, _ = measure_ref(L, R, 5)
    assert np.array_equal(bmp_io.read_bmp(str(img_out / "view_0.bmp")), align_rows_ref(R, *[float(v) for v in st0[1:]]))
