"""The shot-change detector on the GPU (stm_set_cut, stm_cut_detect, the frame calls and the frame stream), bit for bit against the
numpy statement in tests/test_cut_ref.py.  The frame calls' oracle is the same call, detector off, on freshly zeroed states."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_align_ref import displace
from test_balance_ref import distort
from test_cut_ref import STATE_WORDS, detect_ref, edge_pair, score_ref, sig_ref
from test_packing_ref import unpack_nv12_ref, unpack_ref

pytestmark = pytest.mark.gpu

FILL = 0x77
D, ZD = 16, 8
ONE = 0x3F800000  # 1.0f: the `valid` word of a float state
THRESH = 370


@pytest.fixture(autouse=True)
def _settings_off_afterwards(gpu_ready):
    from stm_amd import device_api as dev
    assert dev.get_cut()[0] == 0
    yield
    assert dev.get_cut()[0] == 0, "a test left the thread's detector on"
    assert dev.get_balance()[0] == 0 and dev.get_align()[0] == 0 and dev.get_packing() == dev.PACKING_OFF


@pytest.fixture
def lib(stm, gpu_ready):
    import torch
    l = stm.lib()
    l.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return l


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _zero_state():
    import torch
    return torch.zeros(STATE_WORDS, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------- 1. the stage
SHAPES = [(4, 4), (5, 7), (16, 16), (16, 17), (37, 61), (67, 130), (513, 520)]
_BUD = []


def _bud(H, W):
    if not _BUD:
        from stm_amd import bmp_io
        _BUD.append(bmp_io.read_bmp(os.path.join(GOLDEN, "bud_2.bmp")))
    b = _BUD[0]
    return np.ascontiguousarray(np.pad(b, ((0, max(H - b.shape[0], 0)), (0, max(W - b.shape[1], 0)), (0, 0)), mode="wrap")[:H, :W])


def _contents(H, W):
    """flat (all lanes share one index), two levels split inside a wave, noise (the fall-through path), a crop of bud_2"""
    flat = np.full((H, W, 3), 93, np.uint8)
    two = np.full((H, W, 3), 20, np.uint8)
    two.reshape(-1, 3)[np.arange(H * W) % 64 >= 37] = 200  # row-major: lanes 37 .. 63 of every wave hold the other level
    noise = np.random.RandomState(H * 1000 + W).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    return [("flat", flat), ("two", two), ("noise", noise), ("bud", _bud(H, W))]


@pytest.mark.parametrize("E", [3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_cut_detect_device(gpu_ready, shape, E):
    """the four contents as one sequence through stm_d_cut_detect: every signature and every state word is the statement's"""
    import torch
    from stm_amd import device_api as dev
    H, W = shape
    state, sig = _zero_state(), torch.full((256,), -1, dtype=torch.int32, device="cuda")
    want = None
    for name, img in _contents(H, W):
        if E == 4:
            img = np.concatenate([img, np.random.RandomState(5).randint(0, 256, size=(H, W, 1)).astype(np.uint8)], axis=2)
        want = detect_ref(img, want, THRESH, 1)
        dev.d_cut_detect(_cuda(img), THRESH, 1, state, sig=sig)
        torch.cuda.synchronize()
        assert np.array_equal(sig.cpu().numpy().view(np.uint32).astype(np.int64), sig_ref(img)), (shape, E, name)
        assert np.array_equal(state.cpu().numpy(), want), (shape, E, name, state.cpu().numpy()[:4], want[:4])
    assert int(want[4:].sum()) == H * W


def _run_sequence(steps, resets=()):
    """steps = [(image, thresh, min_gap)]: the device's state after each"""
    import torch
    from stm_amd import device_api as dev
    state = _zero_state()
    got = []
    for img, th, gap in steps:
        dev.d_cut_detect(_cuda(img), th, gap, state, resets)
        torch.cuda.synchronize()
        got.append(state.cpu().numpy())
    return got


def _ref_sequence(steps):
    st, want = None, []
    for img, th, gap in steps:
        st = detect_ref(img, st, th, gap)
        want.append(st)
    return want


def test_decision_sequences(gpu_ready):
    a = np.full((16, 16, 3), 40, np.uint8)
    b = np.full((16, 16, 3), 250, np.uint8)
    e0, e1 = edge_pair()
    other = np.random.RandomState(3).randint(0, 256, size=(16, 17, 3)).astype(np.uint8)
    seqs = {
        "first, repeat, cut, repeat": [(a, 300, 1), (a, 300, 1), (b, 300, 1), (b, 300, 1)],
        "a suppressed cut": [(a, 300, 3), (a, 300, 3), (a, 300, 3), (b, 300, 3), (a, 300, 3)],
        "edge at 350": [(e0, 350, 1), (e1, 350, 1), (e1, 350, 1)],
        "edge at 351": [(e0, 351, 1), (e1, 351, 1), (e0, 351, 1)],
        "a stale state of another size": [(a, 300, 1), (a, 300, 1), (other, 300, 1), (other, 300, 1), (a, 300, 1)],
    }
    flags = {}
    for name, steps in seqs.items():
        got, want = _run_sequence(steps), _ref_sequence(steps)
        for k in range(len(steps)):
            assert np.array_equal(got[k], want[k]), (name, k, got[k][:4], want[k][:4])
        flags[name] = [int(s[1]) for s in got]
    assert flags["first, repeat, cut, repeat"] == [1, 0, 1, 0]
    assert flags["a suppressed cut"] == [1, 0, 0, 1, 0]
    assert flags["edge at 350"] == [1, 1, 0] and flags["edge at 351"] == [1, 0, 0]
    assert flags["a stale state of another size"] == [1, 0, 1, 0, 1]
    assert score_ref(e0, e1) == 350


@pytest.mark.parametrize("mask", range(8))
def test_resets(gpu_ready, mask):
    """three states preset to 1.0f: all first words are zero after a cut, all untouched after a non-cut; any subset may be null"""
    import torch
    from stm_amd import device_api as dev
    a = np.full((8, 8, 3), 40, np.uint8)
    b = np.full((8, 8, 3), 250, np.uint8)
    words = [torch.full((4,), ONE, dtype=torch.int32, device="cuda").view(torch.float32), torch.full((4,), ONE, dtype=torch.int32, device="cuda").view(torch.float32),
             torch.full((769,), ONE, dtype=torch.int32, device="cuda")]
    resets = [w if (mask >> k) & 1 else None for k, w in enumerate(words)]
    state = _zero_state()
    dev.d_cut_detect(_cuda(a), 300, 1, state)  # the first frame, without resets
    dev.d_cut_detect(_cuda(a), 300, 1, state, resets)  # a non-cut
    torch.cuda.synchronize()
    assert state.cpu().numpy()[1] == 0
    for w in words:
        assert (w.view(torch.int32) == ONE).all()
    dev.d_cut_detect(_cuda(b), 300, 1, state, resets)  # a cut
    torch.cuda.synchronize()
    assert state.cpu().numpy()[1] == 1
    for k, w in enumerate(words):
        v = w.view(torch.int32).cpu().numpy()
        assert v[0] == (0 if (mask >> k) & 1 else ONE) and (v[1:] == ONE).all(), (mask, k)


def test_host_flavour_equals_the_device_flavour(gpu_ready):
    from stm_amd import host_api as host
    H, W = 37, 61
    steps = [(img, THRESH, 2) for _, img in _contents(H, W)]
    dev_states = _run_sequence(steps)
    st = None
    for k, (img, th, gap) in enumerate(steps):
        before = None if st is None else st.copy()
        cut, new = host.cut_detect(img, th, gap, st)
        assert before is None or np.array_equal(st, before)  # nothing passed in is modified
        assert cut == int(new[1]) and np.array_equal(new, dev_states[k]), k
        st = new


# ------------------------------------------------------------------------------------------------------- 2. the frame calls
_SHOTS = {}


def _shot(H, W, which):
    """two synthetic shots with different content, disparity ranges, vertical offsets and right-eye tones"""
    from stm_amd import synth
    if (H, W, which) not in _SHOTS:
        if which == "A":
            L, R, _ = synth.stereo_pair(H, W, D, ZD, seed=77)
            R = distort(displace(R, 1.4, 0.0, 0.0), (0.9, 0.95, 1.0), (4, 0, -3), (1.0, 1.0, 1.0))
        else:
            L, R, _ = synth.stereo_pair(H, W, 6, 1, seed=5)
            L = np.clip(L.astype(np.int32) * 0.5 + 120, 0, 255).astype(np.uint8)
            R = np.clip(R.astype(np.int32) * 0.5 + 120, 0, 255).astype(np.uint8)
            R = distort(displace(R, -2.2, 0.0, 0.0), (1.1, 0.85, 0.9), (-8, 6, 10), (1.0, 1.0, 1.0))
        L, R = np.ascontiguousarray(L), np.ascontiguousarray(R)
        L.setflags(write=False)
        R.setflags(write=False)
        _SHOTS[(H, W, which)] = (L, R)
    return _SHOTS[(H, W, which)]


def _params():
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=ZD, usd=17, lsd=8)


def _frame_call(kind, inp, H, W, stages=3, reduced=None):
    """one frame call with the thread's settings as they are; kind "bgr": a side-by-side or packed BGR frame, "nv12": (y, uv)"""
    import torch
    from stm_amd import device_api as dev
    p = _params()
    dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    dr, out = torch.zeros_like(dl), torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    if kind == "nv12":
        il = torch.full((H, W, 3), FILL, dtype=torch.uint8, device="cuda")
        dev.d_adcensus_stm_nv12(_cuda(inp[0]), _cuda(inp[1]), dl, dr, out, p, stages, 0, il, torch.full_like(il, FILL))
    elif reduced is not None:
        dev.d_adcensus_stm_2s(_cuda(inp), dl, dr, out, p, reduced[0], reduced[1], reduced[2], stages)
    else:
        dev.d_adcensus_stm(_cuda(inp), dl, dr, out, p, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


FORMS = {
    "bgr": None,
    "nv12": None,
    "half_linear": (1, 0, 0, 0),
    "half_catmull": (1, 0, 1, 0),
    "tab_half": (3, 0, 0, 0),
    "swap": (0, 1, 0, 0),
    "gap": (0, 0, 0, 6),
}


def _form(name, L, R):
    """(kind, the call's input, packing, the unpacked left eye as the statement sees it)"""
    from stm_amd import synth
    H, W = L.shape[:2]
    if name == "bgr":
        return "bgr", np.ascontiguousarray(np.concatenate([L, R], axis=1)), None, L
    if name == "nv12":
        y, uv = synth.bgr_to_nv12(np.concatenate([L, R], axis=1), 0)
        return "nv12", (y, uv), None, unpack_nv12_ref(y, uv, H, W, (0, 0, 0), 0, 0)[0]
    pk = FORMS[name]
    f = synth.pack_frame(L, R, pk[0], pk[1], pk[3], fill=0x33)
    return "bgr", f, pk, unpack_ref(f, H, W, pk[:3], pk[3])[0]


@pytest.mark.parametrize("form", list(FORMS))
def test_frame_call_sees_the_left_eye_in_every_input_form(gpu_ready, form):
    """two frame calls at 48 x 96 under mode 1: the state is the statement's on the unpacked, converted left eye"""
    import torch
    from stm_amd import device_api as dev
    H, W = 48, 96
    state = _zero_state()
    want = None
    for which in ("A", "B"):
        kind, inp, pk, eye_l = _form(form, *_shot(H, W, which))
        want = detect_ref(eye_l, want, THRESH, 1)
        if pk is not None:
            dev.set_packing(*pk)
        dev.set_cut(1, THRESH, 1, state)
        try:
            _frame_call(kind, inp, H, W, 3)
        finally:
            dev.set_cut(0)
            dev.set_packing(0, 0, 0, 0)
        torch.cuda.synchronize()
        assert np.array_equal(state.cpu().numpy(), want), (form, which, state.cpu().numpy()[:4], want[:4])
    assert want[1] == 1  # the two shots are a cut at the default threshold


class _States:
    """the thread's depth, alignment and balance in mode 2 at rate 0.25 on device states of their own, for those named in `which`"""

    def __init__(self, which):
        import torch
        self.which = which
        self.depth = torch.zeros(4, dtype=torch.float32, device="cuda")
        self.align = torch.zeros(4, dtype=torch.float32, device="cuda")
        self.balance = torch.zeros(769, dtype=torch.int32, device="cuda")

    def __enter__(self):
        from stm_amd import device_api as dev
        if "depth" in self.which:
            dev.set_depth_auto(-2.0, 2.0, 4.0, 20, 0.25, self.depth)
            dev.set_depth(2)
        if "align" in self.which:
            dev.set_align_auto(8, 0.25, self.align)
            dev.set_align(2)
        if "balance" in self.which:
            dev.set_balance_auto(64, 0.25, self.balance)
            dev.set_balance(2)
        return self

    def __exit__(self, *exc):
        from stm_amd import device_api as dev
        dev.set_depth(0)
        dev.set_depth_auto(-1.0, 1.0, 1.0, 20, 1.0, None)
        dev.set_align(0)
        dev.set_align_auto(16, 1.0, None)
        dev.set_balance(0)
        dev.set_balance_auto(48, 1.0, None)


def _sequence(which, frames, call, detector):
    """the outputs of the frame calls on `frames`, the states carried from frame to frame; detector: with stm_set_cut on"""
    from stm_amd import device_api as dev
    outs, flags = [], []
    cut_state = _zero_state()
    with _States(which):
        for f in frames:
            if detector:
                dev.set_cut(1, THRESH, 1, cut_state)
            try:
                outs.append(call(f))
            finally:
                dev.set_cut(0)
            flags.append(int(cut_state.cpu().numpy()[1]))
    return outs, flags


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


CASES = [("depth", "bgr"), ("align", "bgr"), ("balance", "bgr"), ("depth align balance", "bgr"), ("depth align balance", "2s"),
         ("depth align balance", "nv12")]


@pytest.mark.parametrize("case", CASES, ids=["%s-%s" % (c[0].replace(" ", "+"), c[1]) for c in CASES])
def test_states_restart_at_a_cut(gpu_ready, case):
    """A, A, B, B at 48 x 96, D = 16, the states in mode 2 at rate 0.25.  With the detector on the third frame is the call on B with
    freshly zeroed states; with it off it is not (so the inputs discriminate).  The second frame equals the run without the detector.
    The fourth frame continues from the restart: it equals the second frame of a detector-less run that begins at B -- the states of
    the two runs differ from the third frame on, so the fourth frames of the two runs of A, A, B, B differ as well (asserted)."""
    from stm_amd import synth
    which, form = case
    H, W = 48, 96

    def inp(shot):
        L, R = _shot(H, W, shot)
        sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
        return synth.bgr_to_nv12(sbs, 0) if form == "nv12" else sbs

    def call(f):
        if form == "nv12":
            return _frame_call("nv12", f, H, W, 3)
        return _frame_call("bgr", f, H, W, 3, reduced=(H // 2, W // 2, 0.5) if form == "2s" else None)
    A, B = inp("A"), inp("B")
    on, flags = _sequence(which, [A, A, B, B], call, True)
    off, none = _sequence(which, [A, A, B, B], call, False)
    fresh, _ = _sequence(which, [B, B], call, False)
    assert flags == [1, 0, 1, 0] and none == [0, 0, 0, 0]
    assert _equal(on[0], off[0]) and _equal(on[1], off[1])
    assert _equal(on[2], fresh[0]), case
    assert not _equal(off[2], fresh[0]), case  # the inputs discriminate: the old shot's numbers reach the new shot
    assert _equal(on[3], fresh[1]), case
    assert not _equal(off[3], fresh[1]), case
    assert fresh[0][0].any() and fresh[0][2].any()


def test_null_states_are_not_passed(gpu_ready):
    """mode 2 with scratch states (null d_state) under the detector: nothing to reset, the frames are those without the detector"""
    from stm_amd import device_api as dev
    H, W = 48, 96
    frames = [np.ascontiguousarray(np.concatenate(_shot(H, W, s), axis=1)) for s in ("A", "B")]
    outs = {}
    for detector in (False, True):
        cut_state = _zero_state()
        dev.set_depth_auto(-2.0, 2.0, 4.0, 20, 0.25, None)
        dev.set_depth(2)
        dev.set_align_auto(8, 0.25, None)
        dev.set_align(2)
        dev.set_balance_auto(64, 0.25, None)
        dev.set_balance(2)
        try:
            if detector:
                dev.set_cut(1, THRESH, 1, cut_state)
            outs[detector] = [_frame_call("bgr", f, H, W, 3) for f in frames]
        finally:
            dev.set_cut(0)
            dev.set_depth(0)
            dev.set_depth_auto(-1.0, 1.0, 1.0, 20, 1.0, None)
            dev.set_align(0)
            dev.set_align_auto(16, 1.0, None)
            dev.set_balance(0)
            dev.set_balance_auto(48, 1.0, None)
    assert all(_equal(a, b) for a, b in zip(outs[False], outs[True]))


def off_outputs():
    """every frame call of this file with the detector never set or set to mode 0 (the caller decides): a digest of the outputs"""
    import hashlib
    from stm_amd import synth
    H, W = 48, 96
    h = hashlib.sha256()
    for form in FORMS:
        kind, inp, pk, _ = _form(form, *_shot(H, W, "A"))
        from stm_amd import device_api as dev
        if pk is not None:
            dev.set_packing(*pk)
        try:
            for o in _frame_call(kind, inp, H, W, 3):
                h.update(o.tobytes())
        finally:
            dev.set_packing(0, 0, 0, 0)
    sbs = np.ascontiguousarray(np.concatenate(_shot(H, W, "B"), axis=1))
    with _States("depth align balance"):
        for o in _frame_call("bgr", sbs, H, W, 3) + _frame_call("bgr", sbs, H, W, 3, reduced=(H // 2, W // 2, 0.5)) + \
                _frame_call("nv12", synth.bgr_to_nv12(sbs, 0), H, W, 3):
            h.update(o.tobytes())
    return h.hexdigest()


def test_mode_0_is_a_process_that_never_set_the_detector(gpu_ready):
    from stm_amd import device_api as dev
    state = _zero_state()
    dev.set_cut(1, THRESH, 1, state)
    dev.set_cut(0)
    here = off_outputs()
    assert (state == 0).all()
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_cut as t\n"
            "print('digest', t.off_outputs())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ("digest " + here) in r.stdout, r.stdout + r.stderr


def test_frame_rules(gpu_ready, lib):
    """a frame smaller than 4 x 4 is refused while the mode is 1, with nothing written; with the mode 0 it is taken"""
    import torch
    from stm_amd import device_api as dev
    lib.stm_set_error_mode(1)
    try:
        p = _params()
        H, W = 3, 16
        sbs = torch.zeros((H, 2 * W, 3), dtype=torch.uint8, device="cuda")
        dl = torch.full((H, W), 5.0, dtype=torch.float32, device="cuda")
        dr, out = torch.full_like(dl, 5.0), torch.full((H, W, 3), FILL, dtype=torch.uint8, device="cuda")
        state = _zero_state()
        dev.set_cut(1, THRESH, 1, state)
        try:
            lib.stm_d_adcensus_stm(sbs.data_ptr(), dl.data_ptr(), dr.data_ptr(), out.data_ptr(), H, 2 * W, W, H, W, 3, p.num_views, p.angle,
                                   p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, 3)
            msg = lib.stm_last_error()
            lib.stm_d_adcensus_stm_2s(sbs.data_ptr(), dl.data_ptr(), dr.data_ptr(), out.data_ptr(), H, 2 * W, W, H, W, 2, 8, 3, C.c_float(0.5),
                                      p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                                      p.thresh_s, p.thresh_h, 3)
            msg2 = lib.stm_last_error()
        finally:
            dev.set_cut(0)
        torch.cuda.synchronize()
        assert b"d_adcensus_stm" in msg and b"shot-change" in msg and b">= 4" in msg, msg
        assert b"d_adcensus_stm_2s" in msg2 and b"shot-change" in msg2, msg2
        assert (dl == 5.0).all() and (out == FILL).all() and (state == 0).all()
    finally:
        lib.stm_set_error_mode(0)


# ------------------------------------------------------------------------------------------------------- 3. the frame stream
def stream_check():
    """A A A A B B B B through a stream with the detector and the three states in mode 2 at rate 0.25: the flags, the scores, and every
    frame against the thread-API sequence.  Returns a digest of the outputs (the caller compares graphs on with graphs off)."""
    import hashlib
    from stm_amd import device_api as dev, video
    H, W = 48, 96
    shots = {s: _shot(H, W, s) for s in "AB"}
    order = "AAAABBBB"
    frames = [np.ascontiguousarray(np.concatenate(shots[s], axis=1)) for s in order]
    fs = video.FrameStream(H, W, _params(), cut=(THRESH, 1), depth_auto=(-2.0, 2.0, 4.0, 20, 0.25), align_auto=(8, 0.25),
                           balance_auto=(64, 0.25))
    outs, cuts = [], []
    try:
        assert fs.cut() is None  # -1 before a collect
        pending = 0
        for k, f in enumerate(frames):
            if pending == 2:
                outs.append(fs.collect())
                cuts.append(fs.cut())
                pending -= 1
            fs.submit(f)
            pending += 1
            if k == 0:  # the setter is refused after the first submit (as a return value: error mode 1)
                dev.lib().stm_set_error_mode(1)
                try:
                    with pytest.raises(ValueError, match="only before the first submit"):
                        fs.set_cut(1, THRESH, 1)
                    with pytest.raises(ValueError, match="only before the first submit"):
                        fs.set_cut(0)
                finally:
                    dev.lib().stm_set_error_mode(0)
        while pending:
            outs.append(fs.collect())
            cuts.append(fs.cut())
            pending -= 1
    finally:
        fs.close()
    st, want_cuts = None, []
    for s in order:
        st = detect_ref(shots[s][0], st, THRESH, 1)
        want_cuts.append((int(st[1]), int(st[3]), int(st[2])))
    assert [c[0] for c in cuts] == [1, 0, 0, 0, 1, 0, 0, 0]
    assert cuts == want_cuts, (cuts, want_cuts)
    thread, flags = _sequence("depth align balance", frames, lambda f: _frame_call("bgr", f, H, W, 3), True)
    assert flags == [1, 0, 0, 0, 1, 0, 0, 0]
    h = hashlib.sha256()
    for k in range(len(frames)):
        assert outs[k][0] == k
        for j in range(3):
            assert np.array_equal(outs[k][1 + j], thread[k][j]), (k, j)
            h.update(outs[k][1 + j].tobytes())
    return h.hexdigest()


def test_stream(gpu_ready):
    here = stream_check()
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_cut as t\n"
            "print('digest', t.stream_check())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, STM_STREAM_GRAPH="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ("digest " + here) in r.stdout, r.stdout + r.stderr


def test_stream_rules_and_mode_0(gpu_ready, lib):
    from stm_amd import video
    H, W = 48, 96
    frames = [np.ascontiguousarray(np.concatenate(_shot(H, W, s), axis=1)) for s in "AB"]
    lib.stm_set_error_mode(1)
    try:
        fs = video.FrameStream(H, W, _params())
        try:
            for bad in ((2, THRESH, 1), (-1, THRESH, 1), (1, 0, 1), (1, 1001, 1), (1, THRESH, 0), (1, THRESH, (1 << 20) + 1)):
                with pytest.raises(ValueError):
                    fs.set_cut(*bad)
            fs.set_cut(1, THRESH, 2)
            fs.set_cut(0)  # off again before the first submit
            got = []
            for f in frames:
                fs.submit(f)
                got.append((fs.collect(), fs.cut()))
        finally:
            fs.close()
        small = video.FrameStream(3, 16, _params())
        try:
            with pytest.raises(ValueError, match="shot-change"):
                small.set_cut(1, THRESH, 1)
        finally:
            small.close()
    finally:
        lib.stm_set_error_mode(0)
    for k, (out, cut) in enumerate(got):
        assert cut == (0, 0, 0)
        want = _frame_call("bgr", frames[k], H, W, 3)
        for j in range(3):
            assert np.array_equal(out[1 + j], want[j]), (k, j)


# ------------------------------------------------------------------------------------------------------- 4. the driver
def test_video_cli_lists_the_cuts(gpu_ready, tmp_path):
    from stm_amd import bmp_io
    H, W = 48, 96
    order = "AAABB"
    src = tmp_path / "in"
    src.mkdir()
    for k, s in enumerate(order):
        bmp_io.write_bmp(str(src / ("f_%03d.bmp" % k)), np.ascontiguousarray(np.concatenate(_shot(H, W, s), axis=1)))
    args = [sys.executable, os.path.join(ROOT, "tools", "stm_video.py"), str(src), "8", "18.43", str(W), str(H), str(D), str(ZD),
            "10", "30", "6", "20", "17", "8", "20", "0.4", str(tmp_path / "o")]
    text = subprocess.check_output(args + ["--cut", "--balance-auto", "64", "0.25"]).decode()
    assert "cuts at frames: 0 3\n" in text, text
    st = None
    for k, s in enumerate(order):
        st = detect_ref(_shot(H, W, s)[0], st, THRESH, 3)
        assert "frame %d: cut %d score %d since %d\n" % (k, st[1], st[3], st[2]) in text, (k, text)
    assert subprocess.call(args + ["--cut", "370"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0
