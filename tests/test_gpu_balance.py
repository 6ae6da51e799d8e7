"""The colour balance between the eyes on the GPU (stm_set_balance, stm_balance_fit, stm_balance_apply, the frame calls and the frame
stream), bit for bit against the numpy statement in tests/test_balance_ref.py.  The frame calls' oracle is the same call with the
balance off on the statement's balanced frame."""
import ctypes as C

import numpy as np
import pytest

from test_align_ref import align_frame_ref, displace
from test_balance_ref import apply_ref, balance_frame_ref, distort, fit_ref, hist_ref, lut_ref, tables_ref
from test_packing_ref import unpack_nv12_ref, unpack_ref

pytestmark = pytest.mark.gpu

T = 0x2000
FILL = 0x77
D, ZD = 16, 8
IDENTITY = np.tile(np.arange(256, dtype=np.uint8), (3, 1))


@pytest.fixture(autouse=True)
def _balance_off_afterwards(gpu_ready):
    from stm_amd import device_api as dev
    assert dev.get_balance()[0] == 0
    yield
    assert dev.get_balance()[0] == 0, "a test left the thread's balance on"
    assert dev.get_align()[0] == 0
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


def _noise(H, W, seed, lo=0, hi=256):
    return np.random.RandomState(seed).randint(lo, hi, size=(H, W, 3)).astype(np.uint8)


def _buf(lut):
    return (C.c_uint8 * 768).from_buffer_copy(np.ascontiguousarray(lut, np.uint8).tobytes())


# ------------------------------------------------------------------------------------------------------- 1. the stage: apply
WIDTHS = [1, 2, 3, 17, 63, 64, 65, 130, 257, 300]
ROWS = [1, 2, 3, 4, 5, 33]


def _odd_state():
    """a state whose levels leave 0 .. 255 * 256 on both sides, and sit on both sides of step 7's rounding"""
    rng = np.random.RandomState(11)
    st = np.zeros(769, np.int32)
    st[0] = 1
    st[1:] = rng.randint(-3000, 70000, size=768)
    st[1:9] = [0, 127, 128, 383, 384, 255 * 256 + 127, 255 * 256 + 128, -129]
    return st


def _tables():
    """(name, lut768 or None, state or None)"""
    rng = np.random.RandomState(3)
    st = _odd_state()
    assert (st[1:] < 0).any() and (st[1:] > 255 * 256).any()
    return [("random", rng.randint(0, 256, size=(3, 256)).astype(np.uint8), None), ("identity", IDENTITY, None),
            ("constant", np.repeat(np.array([9, 200, 77], np.uint8), 256).reshape(3, 256), None), ("state", None, st)]


@pytest.mark.parametrize("E", [3, 4])
def test_balance_apply_device(lib, E):
    """every width 1 .. 300 (the row count and the table rotating), and every listed width x every row count x every table; caller
    buffers at byte offsets 0 .. 3 (input and output differently), the bytes past a pixel's third left alone, nothing outside the
    output written"""
    from test_gpu_caller_buffers import Arena, P, read
    tables = _tables()
    d_state = _cuda(tables[3][2])
    cases = [(W, ROWS[W % len(ROWS)], W % 4) for W in range(1, 301)]
    cases += [(W, H, k) for W in WIDTHS for H in ROWS for k in range(4)]
    n = 0
    for lo in range(0, len(cases), 90):
        arena = Arena(True, nbytes=16 << 20)
        done = []
        for (W, H, k) in cases[lo:lo + 90]:
            name, lut, state = tables[k]
            img = np.full((H, W, E), 0xC3, np.uint8)
            img[:, :, :3] = _noise(H, W, H * 1000 + W)
            d_img = arena.put(img, n % 4)
            d_out = arena.put(np.full((H, W, E), FILL, np.uint8), (n // 4 + n) % 4)
            lib.stm_d_balance_apply(P(d_out), P(d_img), H, W, E, _buf(lut) if lut is not None else None,
                                    d_state.data_ptr() if state is not None else None)
            done.append((name, H, W, img, lut if lut is not None else lut_ref(state), d_out))
            n += 1
        assert arena.intact(), lo
        for name, H, W, img, lut, d_out in done:
            got = read(d_out, np.uint8, (H, W, E))
            assert np.array_equal(got[:, :, :3], apply_ref(img, lut)), (name, H, W, E)
            assert (got[:, :, 3:] == FILL).all(), (name, H, W, E)
    lut = lut_ref(tables[3][2]).reshape(768)
    assert lut[:8].tolist() == [0, 0, 1, 1, 2, 255, 255, 0] and (lut == 0).sum() > 8 and (lut == 255).sum() > 8  # the clamp was met


def test_balance_apply_host(gpu_ready):
    from stm_amd import host_api as api
    for (H, W, E) in [(5, 65, 3), (33, 130, 4)]:
        img = np.full((H, W, E), 0xC3, np.uint8)
        img[:, :, :3] = _noise(H, W, 9)
        for name, lut, state in _tables():
            got = api.balance_apply(img, lut, state)
            want = apply_ref(img, lut if lut is not None else lut_ref(state))
            assert np.array_equal(got[:, :, :3], want) and (got[:, :, 3:] == 0).all(), (name, H, W, E)
        assert np.array_equal(api.balance_lut(_odd_state()), lut_ref(_odd_state()))


# ------------------------------------------------------------------------------------------------------- 2. the measurement
SHAPES = [(1, 1), (4, 8), (40, 64), (67, 130), (97, 300)]
_MEASURE = {}


def _measure_inputs(H, W):
    """name -> (left, right)"""
    if (H, W) not in _MEASURE:
        noise = _noise(H, W, H + W)
        two = np.where(_noise(H, W, 5) < 90, 40, 200).astype(np.uint8)
        gap = noise.copy()  # the right eye has no level in 100 .. 139: the windows of 108 .. 131 are empty
        gap[(gap >= 100) & (gap < 140)] = 99
        pairs = {"noise": (noise, _noise(H, W, 7)),
                 "flat": (np.full((H, W, 3), 100, np.uint8), np.full((H, W, 3), 120, np.uint8)),
                 "two levels": (np.where(two == 40, 60, 190).astype(np.uint8), two),
                 "gap": (noise, gap),
                 "gain": (noise, distort(noise, (0.8, 0.95, 0.9), (0, 0, 0), (1, 1, 1))),
                 "offset": (noise, distort(noise, (1, 1, 1), (10, -5, 4), (1, 1, 1))),
                 "gamma": (noise, distort(noise, (0.8, 0.95, 0.9), (10, -5, 4), (0.85, 1.1, 1.2)))}
        for pair in pairs.values():
            for a in pair:
                a.setflags(write=False)
        _MEASURE[(H, W)] = pairs
    return _MEASURE[(H, W)]


def test_measure_inputs_are_what_their_names_say():
    p = _measure_inputs(97, 300)
    h = hist_ref(*p["gap"])
    assert (h[1, :, 100:140] == 0).all() and (h[1, :, 99] > 0).all() and (h[1, :, 140] > 0).all()
    assert len(np.unique(p["flat"][1])) == 1 and len(np.unique(p["two levels"][1])) == 2
    t = tables_ref(hist_ref(*p["gain"]), 255)
    assert (t[0, 200] > 200 + 5) and not np.array_equal(tables_ref(hist_ref(*p["gain"]), 5), t)


@pytest.mark.parametrize("max_shift", [0, 5, 255])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_balance_fit_device(gpu_ready, shape, max_shift):
    """the histograms as integers through d_hist, the state as integers; 3- and 4-byte pixels"""
    import torch
    from stm_amd import device_api as dev
    H, W = shape
    for k, (name, (left, right)) in enumerate(sorted(_measure_inputs(H, W).items())):
        E = 3 + k % 2
        imgs = []
        for v in (left, right):
            a = np.full((H, W, E), 0x3C, np.uint8)
            a[:, :, :3] = v
            imgs.append(_cuda(a))
        state = torch.zeros(769, dtype=torch.int32, device="cuda")
        hist = torch.full((1536,), -1, dtype=torch.int32, device="cuda")
        dev.d_balance_fit(imgs[0], imgs[1], max_shift, 1.0, state, hist)
        torch.cuda.synchronize()
        h, want = fit_ref(left, right, max_shift)
        assert np.array_equal(hist.cpu().numpy().astype(np.int64).reshape(2, 3, 256), h), (name, "histograms")
        got = state.cpu().numpy()
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:8])
        if max_shift == 0:
            assert np.array_equal(lut_ref(got), IDENTITY)


def test_balance_fit_recursive_update_and_host_flavour(gpu_ready):
    """three frames through one state at rate 0.5, device and host flavour; without d_hist"""
    import torch
    from stm_amd import device_api as dev, host_api as api
    H, W = 67, 130
    pairs = _measure_inputs(H, W)
    seq = [pairs["gain"], pairs["gamma"], pairs["offset"]]
    state = torch.zeros(769, dtype=torch.int32, device="cuda")
    want, host = None, None
    for left, right in seq:
        dev.d_balance_fit(_cuda(left), _cuda(right), 64, 0.5, state)
        torch.cuda.synchronize()
        _, want = fit_ref(left, right, 64, 0.5, want)
        assert np.array_equal(state.cpu().numpy(), want)
        host = api.balance_fit(left, right, 64, 0.5, host)
        assert np.array_equal(host, want)
    _, alone = fit_ref(seq[2][0], seq[2][1], 64)
    assert want[0] == 1 and not np.array_equal(want, alone)  # the history took part


# ------------------------------------------------------------------------------------------------------- 3. the frame calls
_PAIRS = {}
FIELD = (2.6, 0.011, -0.017)
SETTING = ((0.8, 0.95, 0.9), (10, -5, 4), (0.85, 1.1, 1.2))
GIVEN = np.stack([np.clip(np.arange(256) * g + o, 0, 255).astype(np.uint8) for g, o in ((1.2, -9), (1.05, 4), (1.1, -3))])


def _pair(H, W, k=0):
    """frame k of a small sequence: one synthetic stereo pair under fresh noise of +-2 per channel, its right eye darker and
    tinted, a little more in every frame"""
    from stm_amd import synth
    if (H, W, k) not in _PAIRS:
        L, R, _ = synth.stereo_pair(H, W, D, ZD, seed=77)
        rng = np.random.RandomState(k)
        L = np.clip(L.astype(np.int32) + rng.randint(-2, 3, size=L.shape), 0, 255).astype(np.uint8)
        R = np.clip(R.astype(np.int32) + rng.randint(-2, 3, size=R.shape), 0, 255).astype(np.uint8)
        gain = tuple(g - 0.03 * k for g in SETTING[0])
        R = distort(R, gain, SETTING[1], SETTING[2])
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


class _Balanced:
    """the thread's balance (and, with align, a manual alignment) for the duration of a block; mode 2 with a device state or None"""

    def __init__(self, mode, lut=None, max_shift=64, rate=1.0, state=None, align=None):
        self.args = (mode, lut, max_shift, rate, state, align)

    def __enter__(self):
        from stm_amd import device_api as dev
        mode, lut, max_shift, rate, state, align = self.args
        if mode == 2:
            dev.set_balance_auto(max_shift, rate, state)
        dev.set_balance(mode, lut if mode == 1 else None)
        if align is not None:
            dev.set_align(1, *align)

    def __exit__(self, *exc):
        from stm_amd import device_api as dev
        dev.set_align(0)
        dev.set_balance_auto(48, 1.0, None)
        dev.set_balance(0)


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


def _tables_for(mode, eye_l, eye_r, state=None, rate=1.0):
    """(the tables the statement applies, the statement's new state)"""
    if mode == 1:
        return GIVEN, None
    _, st = fit_ref(eye_l, eye_r, 64, rate, state)
    return lut_ref(st), st


@pytest.mark.parametrize("aligned", [False, True], ids=["balance", "align+balance"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case", [("bgr", 48, 96), ("bgr", 67, 130), ("nv12", 48, 96), ("half", 48, 96), ("half", 67, 132)],
                         ids=lambda c: "%s_%dx%d" % c)
def test_frame_under_balance_is_the_plain_frame_on_the_balanced_pair(gpu_ready, case, mode, aligned):
    """stm_d_adcensus_stm / _nv12 at stages 3 and 3 | 0x200 | 0x400 | 0x800, and _2s (BGR); mode 2 with a null state.  With a
    manual alignment on as well the order is fixed: align, then measure and balance the aligned pair."""
    from stm_amd import device_api as dev
    fmt, H, W = case
    L, R = _pair(H, W)
    if aligned:
        R = displace(R, *FIELD)
    kind, inp, pk, (eye_l, eye_r) = _inputs(fmt, L, R)
    raw_r = eye_r
    if aligned:
        eye_r = np.ascontiguousarray(align_frame_ref(eye_l, raw_r, *FIELD)[:, W:])
    lut, _ = _tables_for(mode, eye_l, eye_r)
    assert not np.array_equal(lut, IDENTITY)
    balanced = balance_frame_ref(eye_l, eye_r, lut)
    assert not np.array_equal(balanced[:, W:], eye_r)
    if aligned:  # the other order gives another frame: the check distinguishes them
        lut_o, _ = _tables_for(mode, eye_l, raw_r)
        assert not np.array_equal(align_frame_ref(eye_l, apply_ref(raw_r, lut_o), *FIELD), balanced)
    before = _frame_call(kind, inp, H, W, 3) if pk is None else None
    for stages in (3, 3 | 0x200 | 0x400 | 0x800):
        want = _frame_call("bgr", balanced, H, W, stages)
        if pk is not None:
            dev.set_packing(*pk)
        try:
            with _Balanced(mode, GIVEN, align=FIELD if aligned else None):
                got = _frame_call(kind, inp, H, W, stages)
        finally:
            dev.set_packing(0, 0, 0, 0)
        _same(got, want, (case, mode, stages))
        if kind == "nv12":  # the split images the call hands out are the balanced eyes
            assert np.array_equal(got[3], balanced[:, :W]) and np.array_equal(got[4], balanced[:, W:])
    if fmt == "bgr":
        red = (H // 2, W // 2, 0.5)
        want = _frame_call("bgr", balanced, H, W, 3, reduced=red)
        with _Balanced(mode, GIVEN, align=FIELD if aligned else None):
            got = _frame_call("bgr", inp, H, W, 3, reduced=red)
        _same(got, want, (case, mode, "_2s"))
    if pk is None:  # off again: the bytes of the call before any balance was set, which are not the balanced frame's
        after = _frame_call(kind, inp, H, W, 3)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        assert not np.array_equal(after[2], _frame_call("bgr", balanced, H, W, 3)[2])


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("fmt", ["bgr", "half"])
def test_temporal_history_goes_through_the_current_tables(gpu_ready, fmt, mode):
    """0x2000 through _t: the previous frame is balanced with the CURRENT frame's tables; mode 2 with a device state carried over
    from the previous frame at rate 0.5, so the current tables differ from what either frame alone would give"""
    import torch
    from stm_amd import device_api as dev
    H, W = 48, 96
    (kind, prev_in, pk, prev_eyes), (_, cur_in, _, cur_eyes) = _inputs(fmt, *_pair(H, W, 0)), _inputs(fmt, *_pair(H, W, 3))
    state, st1 = None, None
    if mode == 1:
        lut = GIVEN
    else:
        _, st0 = _tables_for(2, *prev_eyes)
        lut, st1 = _tables_for(2, *cur_eyes, state=st0, rate=0.5)
        assert not np.array_equal(st0, st1) and not np.array_equal(st1, _tables_for(2, *cur_eyes)[1])
        state = _cuda(st0)
    cur_b, prev_b = balance_frame_ref(*cur_eyes, lut), balance_frame_ref(*prev_eyes, lut)
    first = _frame_call("bgr", prev_b, H, W, 2)
    ql, qr = first[0] + np.float32(0.25), first[1] - np.float32(0.25)
    want = _frame_call("bgr", cur_b, H, W, 2 | T, (prev_b, ql, qr))
    assert not np.array_equal(want[0], _frame_call("bgr", cur_b, H, W, 2)[0])  # the step did something
    if pk is not None:
        dev.set_packing(*pk)
    try:
        with _Balanced(mode, GIVEN, rate=0.5, state=state):
            got = _frame_call(kind, cur_in, H, W, 2 | T, (prev_in, ql, qr))
    finally:
        dev.set_packing(0, 0, 0, 0)
    for k in range(2):
        assert np.array_equal(got[k], want[k]), (fmt, mode, k)
    if mode == 2:
        torch.cuda.synchronize()
        assert np.array_equal(state.cpu().numpy(), st1)


def test_frame_rules(gpu_ready, lib):
    """a frame too narrow to hold both eyes is refused with nothing written, under both modes"""
    import torch
    lib.stm_set_error_mode(1)
    try:
        p = _params()
        for mode in (1, 2):
            H, W, Wsbs = 8, 16, 24
            sbs = torch.zeros((H, Wsbs, 3), dtype=torch.uint8, device="cuda")
            dl = torch.full((H, W), 5.0, dtype=torch.float32, device="cuda")
            dr, out = torch.full_like(dl, 5.0), torch.full((H, W, 3), FILL, dtype=torch.uint8, device="cuda")
            with _Balanced(mode, GIVEN):
                lib.stm_d_adcensus_stm(sbs.data_ptr(), dl.data_ptr(), dr.data_ptr(), out.data_ptr(), H, Wsbs, W, H, W, 3, p.num_views, p.angle,
                                       p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, 3)
            msg = lib.stm_last_error()
            torch.cuda.synchronize()
            assert b"d_adcensus_stm" in msg and b"num_cols_sbs" in msg and b"balance" in msg, msg
            assert (dl == 5.0).all() and (out == FILL).all()
    finally:
        lib.stm_set_error_mode(0)


# ------------------------------------------------------------------------------------------------------- 4. the frame stream
def _stream(frames, H, W, late=None, **kw):
    from stm_amd import video
    fs = video.FrameStream(H, W, _params(), **kw)
    outs, tables = [], []
    try:
        pending = 0
        for f in frames:
            if pending == 2:
                outs.append(fs.collect())
                tables.append(fs.balance())
                pending -= 1
            fs.submit(f)
            pending += 1
            if late is not None:
                late(fs)
        while pending:
            outs.append(fs.collect())
            tables.append(fs.balance())
            pending -= 1
    finally:
        fs.close()
    return outs, tables


@pytest.mark.parametrize("mode", [1, 2])
def test_stream_under_balance(gpu_ready, mode):
    """six frames, so that both slots' captured graphs replay: every frame is the plain frame call on the statement's balanced
    frame, and stm_stream_balance reports the statement's tables (mode 2: the state carried from frame to frame at rate 0.5)"""
    from stm_amd import device_api as dev
    H, W, n = 48, 96, 6
    pairs = [_pair(H, W, k) for k in range(n)]
    frames = [np.ascontiguousarray(np.concatenate(pr, axis=1)) for pr in pairs]
    dev.set_balance(1, IDENTITY[:, ::-1])  # the calling thread's own setting never reaches a stream's frames
    try:
        if mode == 1:
            outs, tables = _stream(frames, H, W, balance=GIVEN)
        else:
            outs, tables = _stream(frames, H, W, balance_auto=(64, 0.5))
        plain, off = _stream(frames[:2], H, W)
    finally:
        dev.set_balance(0)
    st = None
    for k in range(n):
        lut, st = _tables_for(mode, *pairs[k], state=st, rate=0.5)
        assert tables[k].shape == (3, 256) and np.array_equal(tables[k], lut), (mode, k)
        want = _frame_call("bgr", balance_frame_ref(pairs[k][0], pairs[k][1], lut), H, W, 3)
        assert outs[k][0] == k
        for j in range(3):
            assert np.array_equal(outs[k][1 + j], want[j]), (mode, k, j)
    if mode == 2:
        assert not np.array_equal(tables[0], tables[n - 1])
    for k in range(2):  # a stream without the setting: today's bytes, whatever the thread has set
        want = _frame_call("bgr", frames[k], H, W, 3)
        assert np.array_equal(off[k], IDENTITY)
        for j in range(3):
            assert np.array_equal(plain[k][1 + j], want[j]), ("off", k, j)


@pytest.fixture
def returning_errors(lib):
    """refusals come back as return values (error mode 1) instead of ending the process"""
    lib.stm_set_error_mode(1)
    try:
        yield lib
    finally:
        lib.stm_set_error_mode(0)


def test_stream_setters_only_before_the_first_submit(returning_errors):
    H, W = 48, 96
    frames = [np.ascontiguousarray(np.concatenate(_pair(H, W, k), axis=1)) for k in range(2)]
    seen = []

    def late(fs):
        for call in (lambda: fs.set_balance(1, GIVEN), lambda: fs.set_balance(2), lambda: fs.set_balance(0),
                     lambda: fs.set_balance_auto(10, 0.5)):
            with pytest.raises(ValueError, match="only before the first submit"):
                call()
            seen.append(1)
    outs, tables = _stream(frames, H, W, late=late, balance=GIVEN)
    assert len(seen) == 8 and all(np.array_equal(t, GIVEN) for t in tables)
    from stm_amd import video
    fs = video.FrameStream(H, W, _params())
    try:
        assert fs.balance() is None  # nothing collected yet
        for bad in (lambda: fs.set_balance(3), lambda: fs.set_balance(1), lambda: fs.set_balance_auto(256, 0.5),
                    lambda: fs.set_balance_auto(8, float("nan")), lambda: fs.set_balance_auto(8, 0.0)):
            with pytest.raises(ValueError):
                bad()
    finally:
        fs.close()
    with pytest.raises(ValueError, match="mutually exclusive"):
        video.FrameStream(H, W, _params(), balance=GIVEN, balance_auto=(48,))


# ------------------------------------------------------------------------------------------------------- 5. the two drivers
def test_video_and_image_cli_with_balance(gpu_ready, tmp_path):
    """tools/stm_video.py --balance-auto MAX_SHIFT RATE on a directory of BMP frames writes the per-frame calls' frames on the
    statement's balanced pairs and prints each frame's tables at three levels; --balance FILE.npy is read by the parser both
    drivers share; tools/stm_image.py --balance-auto hands the balanced right image to its chain (view 0 is the right image); malformed options
    are refused"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from stm_amd import bmp_io, device_api as dev
    H, W, n = 48, 96, 3
    pairs = [_pair(H, W, k) for k in range(n)]
    src = tmp_path / "in"
    src.mkdir()
    for k, pr in enumerate(pairs):
        bmp_io.write_bmp(str(src / ("f_%03d.bmp" % k)), np.ascontiguousarray(np.concatenate(pr, axis=1)))
    out = tmp_path / "o"
    args = [sys.executable, os.path.join(ROOT, "tools", "stm_video.py"), str(src), "8", "18.43", str(W), str(H), str(D), str(ZD),
            "10", "30", "6", "20", "17", "8", "20", "0.4", str(out)]
    p = dev.FrameParams(num_disp=D, zero_disp=ZD, usd=17, lsd=8, angle=18.0)  # the tool truncates the slant

    def frame_on(balanced):
        dl, dr, o = _outputs(H, W)
        dev.d_adcensus_stm(_cuda(balanced), dl, dr, o, p, stages=3)
        return o.cpu().numpy()
    text = subprocess.check_output(args + ["--balance-auto", "64", "0.5"]).decode()
    st = None
    for k in range(n):
        lut, st = _tables_for(2, *pairs[k], state=st, rate=0.5)
        line = "frame %d: balance B %d %d %d G %d %d %d R %d %d %d" % ((k,) + tuple(int(lut[c, v]) for c in range(3) for v in (64, 128, 192)))
        assert line in text, (k, line, text)
        assert np.array_equal(bmp_io.read_bmp(str(out / ("interlaced_%05d.bmp" % k))), frame_on(balance_frame_ref(*pairs[k], lut))), k
    np.save(str(tmp_path / "lut.npy"), GIVEN.reshape(768))
    np.save(str(tmp_path / "short.npy"), GIVEN.reshape(768)[:700])
    np.save(str(tmp_path / "float.npy"), GIVEN.reshape(768).astype(np.float32))
    from stm_amd import video
    for bad in (["--balance"], ["--balance", str(tmp_path / "none.npy")], ["--balance", str(tmp_path / "short.npy")],
                ["--balance", str(tmp_path / "float.npy")], ["--balance-auto", "300", "0.5"], ["--balance-auto", "64", "1.5"],
                ["--balance-auto", "64", "0"], ["--balance-auto", "64", "nan"], ["--balance-auto", "64"],
                ["--balance", str(tmp_path / "lut.npy"), "--balance-auto"]):
        with pytest.raises((ValueError, IndexError)):  # the parser both drivers share ...
            video.take_balance_options(["x"] + bad)
    # ... and a driver ends on its refusal
    assert subprocess.call(args + ["--balance-auto", "64"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0
    rest = ["a", "--balance", str(tmp_path / "lut.npy"), "b"]  # (what FrameStream does with given tables: test_stream_under_balance)
    given, auto = video.take_balance_options(rest)
    assert auto is None and given.shape == (3, 256) and np.array_equal(given, GIVEN) and rest == ["a", "b"]
    rest = ["a", "--balance-auto", "b"]
    assert video.take_balance_options(rest) == (None, (48, 1.0)) and rest == ["a", "b"]
    rest = ["--balance-auto", "7", "0.25", "9"]
    assert video.take_balance_options(rest) == (None, (7, 0.25)) and rest == ["9"]
    L, R = pairs[0]
    bmp_io.write_bmp(str(tmp_path / "l.bmp"), L)
    bmp_io.write_bmp(str(tmp_path / "r.bmp"), R)
    img_out = tmp_path / "i"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "stm_image.py"), str(tmp_path / "l.bmp"), str(tmp_path / "r.bmp"), "10", "30",
                           str(D), str(ZD), "6", "20", "17", "8", "8", "18.43", str(W), str(H), "20", "0.4", str(img_out), "--balance-auto"],
                          stdout=subprocess.DEVNULL)
    _, st0 = fit_ref(L, R, 48)
    assert np.array_equal(bmp_io.read_bmp(str(img_out / "view_0.bmp")), apply_ref(R, lut_ref(st0)))
