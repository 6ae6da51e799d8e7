"""The active picture area on the GPU (stm_set_active, stm_active_detect, stm_active_fill, stm_depth_fit_rect, stm_overlay_fit_rect,
the frame calls and the frame stream), bit for bit against the numpy statement in tests/test_active_ref.py.  A frame call's oracle
is the same call with the setting off, followed by the stage calls applied by hand to its maps; its frame is the numpy render from
those maps and that state."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_active_ref import (STATE_WORDS, counts_ref, depth_fit_rect_ref, detect_ref, fill_ref, frame_with, growth_sequence, overlay_fit_rect_ref,
                             paint_bars, rect_of, ref_step, run_sequence, seq_frame)
from test_cut_ref import detect_ref as cut_ref
from test_depth_ref import depth_fit_ref, render_depth_ref
from test_lens_ref import render_chain
from test_overlay_fit_ref import overlay_fit_ref, state_disparity_ref
from test_packing_ref import unpack_nv12_ref, unpack_ref

pytestmark = pytest.mark.gpu

f32 = np.float32
D, ZD = 16, 8
NAN = float("nan")


@pytest.fixture(autouse=True)
def _settings_off_afterwards(gpu_ready):
    from stm_amd import device_api as dev
    assert dev.get_active()[0] == 0
    yield
    assert dev.get_active()[0] == 0, "a test left the thread's active area on"
    assert dev.get_cut()[0] == 0 and dev.get_packing() == dev.PACKING_OFF and dev.get_overlay()[0] == 0 and dev.get_overlay_auto()[0] == 0


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


def _rect(r):
    import torch
    return None if r is None else torch.tensor(list(r), dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------- 1. the measurement
SHAPES = [(1, 1), (4, 4), (5, 7), (16, 17), (37, 61), (64, 64), (65, 129), (67, 130), (513, 520)]
_BUD = []


def _bud(H, W):
    if not _BUD:
        from stm_amd import bmp_io
        _BUD.append(bmp_io.read_bmp(os.path.join(GOLDEN, "bud_2.bmp")))
    b = _BUD[0]
    return np.ascontiguousarray(np.pad(b, ((0, max(H - b.shape[0], 0)), (0, max(W - b.shape[1], 0)), (0, 0)), mode="wrap")[:H, :W])


def _contents(H, W):
    """flat above and below the threshold, bars on one, two and four sides of widths 1, 63, 64 and 65 (where they leave a picture),
    noise, a crop of bud_2, and a frame whose only lit pixels are one row and one column"""
    out = [("flat_lit", np.full((H, W, 3), 25, np.uint8)), ("flat_dark", np.full((H, W, 3), 24, np.uint8))]
    for w in (1, 63, 64, 65):
        if w < H:
            out.append(("top%d" % w, frame_with(H, W, w, 0, 0, 0, seed=w)))
        if w < W:
            out.append(("right%d" % w, frame_with(H, W, 0, 0, 0, w, seed=w + 1)))
        if 2 * w < H:
            out.append(("top_bottom%d" % w, frame_with(H, W, w, w, 0, 0, seed=w + 2)))
        if 2 * w < H and 2 * w < W:
            out.append(("four%d" % w, frame_with(H, W, w, w, w, w, seed=w + 3)))
    out.append(("noise", np.random.RandomState(H * 1000 + W).randint(0, 256, size=(H, W, 3)).astype(np.uint8)))
    out.append(("bud", _bud(H, W)))
    cross = np.zeros((H, W, 3), np.uint8)
    cross[H // 2, :] = 200
    cross[:, W // 3] = 200
    out.append(("cross", cross))
    return out


@pytest.mark.parametrize("E", [3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_active_detect_device(gpu_ready, shape, E):
    """the contents as one sequence through stm_d_active_detect at hold 2: every count and every state word is the statement's"""
    import torch
    from stm_amd import device_api as dev
    H, W = shape
    state, counts = _zero_state(), torch.full((H + W,), -1, dtype=torch.int32, device="cuda")
    want = None
    kw = dict(thresh_luma=24, lit_permille=10, max_bar_permille=450, hold=2)
    seen = set()
    for name, img in _contents(H, W):
        if E == 4:
            img = np.concatenate([img, np.random.RandomState(5).randint(0, 256, size=(H, W, 1)).astype(np.uint8)], axis=2)
        want, c = detect_ref(img, want, **kw)
        dev.d_active_detect(_cuda(img), state, counts=counts, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy().view(np.uint32).astype(np.int64), c), (shape, E, name)
        assert np.array_equal(state.cpu().numpy(), want), (shape, E, name, state.cpu().numpy(), want)
        seen.add(rect_of(want))
    assert H * W == 1 or len(seen) > 1


def _dev_step(hold):
    """detect(img, state, restart, cut_flag) -> state through the device state; the cut flag travels as word 1 of a cut state"""
    import torch
    from stm_amd import device_api as dev
    d_state = _zero_state()
    cut = torch.zeros(260, dtype=torch.int32, device="cuda")

    def step(img, st, restart, cut_flag):
        d_state.copy_(torch.from_numpy(np.asarray(st, np.int32)))
        cut[1] = int(cut_flag)
        dev.d_active_detect(_cuda(img), d_state, 24, 10, 300, hold, restart, cut_state=cut)
        torch.cuda.synchronize()
        return d_state.cpu().numpy()
    return step


def test_sequences_through_the_device_state(gpu_ready):
    blank = np.zeros((40, 64, 3), np.uint8)
    other = frame_with(40, 65, 9, 0, 0, 0, seed=1)
    seqs = {
        "growth, hold 3": (3, growth_sequence()),
        "a lit frame restarts the run": (3, [(seq_frame(t, seed=i), False, 0) for i, t in enumerate([0, 6, 6, 0, 6, 6, 6])]),
        "hold 1": (1, [(seq_frame(t, seed=i), False, 0) for i, t in enumerate([0, 6, 8, 5, 0, 7])]),
        "each side on its own": (2, [(seq_frame(0, seed=0), False, 0), (seq_frame(4, 6, 10, 12, seed=1), False, 0),
                                     (seq_frame(4, 0, 10, 14, seed=2), False, 0), (seq_frame(4, 6, 9, 12, seed=3), False, 0)]),
        "blank with and without history": (4, [(blank, False, 0), (seq_frame(5, seed=0), False, 0), (seq_frame(9, seed=1), False, 0),
                                               (blank, False, 0), (seq_frame(9, seed=2), False, 0), (blank, True, 0), (seq_frame(7, seed=3), False, 0),
                                               (blank, False, 1)]),
        "restart by the argument and by the flag": (5, [(seq_frame(0, seed=0), False, 0), (seq_frame(6, 3, seed=1), False, 0),
                                                        (seq_frame(6, 3, seed=1), True, 0), (seq_frame(2, 3, seed=2), False, 0),
                                                        (seq_frame(8, 0, seed=3), False, 1)]),
        "a state of another size": (5, [(seq_frame(5, seed=0), False, 0), (other, False, 0), (seq_frame(5, seed=0), False, 0)]),
        "the cap": (1, [(frame_with(40, 64, 18, 18, 30, 30, seed=4), False, 0)]),
    }
    tops = {}
    for name, (hold, frames) in seqs.items():
        got, want = run_sequence(frames, _dev_step(hold)), run_sequence(frames, ref_step(hold))
        for k in range(len(frames)):
            assert np.array_equal(got[k], want[k]), (name, k, got[k], want[k])
        tops[name] = [int(s[1]) for s in got]
    assert tops["growth, hold 3"] == [0, 0, 0, 5, 5, 2, 2, 2, 5, 5]
    assert tops["hold 1"] == [0, 6, 8, 5, 0, 7]
    assert tops["restart by the argument and by the flag"] == [0, 0, 6, 2, 8]
    assert tops["the cap"] == [12]


def test_the_cut_flag_of_a_real_cut_state_restarts_the_fit(gpu_ready):
    import torch
    from stm_amd import device_api as dev
    a0, a1 = seq_frame(0, seed=0), seq_frame(0, seed=0)
    b = np.full((40, 64, 3), 250, np.uint8)
    b[:6] = 3
    frames = [a0, a1, b, b]
    cut, state = torch.zeros(260, dtype=torch.int32, device="cuda"), _zero_state()
    want_cut, want, flags, tops = None, None, [], []
    for img in frames:
        dev.d_cut_detect(_cuda(img), 370, 1, cut)
        dev.d_active_detect(_cuda(img), state, 24, 10, 300, 5, cut_state=cut)
        torch.cuda.synchronize()
        want_cut = cut_ref(img, want_cut, 370, 1)
        want = detect_ref(img, want, 24, 10, 300, 5, cut_flag=int(want_cut[1]))[0]
        assert np.array_equal(cut.cpu().numpy(), want_cut) and np.array_equal(state.cpu().numpy(), want)
        flags.append(int(want_cut[1]))
        tops.append(int(want[1]))
    assert flags == [1, 0, 1, 0] and tops == [0, 0, 6, 6]  # held for 5 frames without the flag, taken at once with it


def test_host_flavour_equals_the_device_flavour(gpu_ready):
    from stm_amd import host_api as host
    frames = growth_sequence()
    want = run_sequence(frames, ref_step(3))
    st = None
    for k, (img, _, _) in enumerate(frames):
        before = None if st is None else st.copy()
        changed, new = host.active_detect(img, hold=3, state=st)
        assert before is None or np.array_equal(st, before)  # nothing passed in is modified
        assert changed == int(new[5]) and np.array_equal(new, want[k]), k
        st = new


# ------------------------------------------------------------------------------------------------------- 2. the consumers
def _rects(H, W):
    return [("full", (0, H, 0, W)), ("one_wide", (0, H, W // 2, W // 2 + 1)), ("one_high", (H // 3, H // 3 + 1, 0, W)),
            ("off_centre", (H // 5, H - 1, 1, (2 * W) // 3 + 1))]


def _pattern(H, W, seed):
    rng = np.random.RandomState(seed)
    d = (rng.randint(-60, 60, size=(H, W)) * 0.25).astype(f32)
    d.ravel()[rng.randint(0, H * W, 5)] = NAN
    return d


@pytest.mark.parametrize("shape", [(16, 17), (37, 61), (67, 130), (513, 520)], ids=lambda s: "%dx%d" % s)
def test_active_fill(gpu_ready, shape):
    import torch
    from stm_amd import device_api as dev, host_api as host
    H, W = shape
    src = _pattern(H, W, 3)
    for name, rect in _rects(H, W):
        d = _cuda(src)
        dev.d_active_fill(d, _rect(rect), -7.5)
        torch.cuda.synchronize()
        got, want = d.cpu().numpy(), fill_ref(src, rect, -7.5)
        assert got.tobytes() == want.tobytes(), (shape, name)
        t, b, l, r = rect
        assert got[t:b, l:r].tobytes() == src[t:b, l:r].tobytes()  # the inside bit for bit, NaNs included
        if H <= 67:
            assert host.active_fill(src, rect, -7.5).tobytes() == want.tobytes()
    d = _cuda(src)
    dev.d_active_fill(d, None, 1.0)
    dev.d_active_fill(d, _rect((-5, H + 9, -1, W + 3)), 1.0)  # clamped to the map: the full rectangle, nothing written
    torch.cuda.synchronize()
    assert d.cpu().numpy().tobytes() == src.tobytes()


@pytest.mark.parametrize("shape", [(16, 17), (37, 61), (67, 130)], ids=lambda s: "%dx%d" % s)
def test_depth_fit_rect(gpu_ready, shape):
    import torch
    from stm_amd import device_api as dev, host_api as host
    H, W = shape
    dl, dr = _pattern(H, W, 4), _pattern(H, W, 5)
    dl[:H // 5], dr[H - 1:] = -15.0, 14.0  # what the off-centre rectangle leaves out
    args = (-4.0, 4.0, 2.0, 20, 0.5)
    for name, rect in _rects(H, W):
        st, want = torch.zeros(4, dtype=torch.float32, device="cuda"), np.zeros(4, f32)
        for step in range(2):  # without and with history
            dev.d_depth_fit_rect(_cuda(dl), _cuda(dr), *args, st, _rect(rect))
            torch.cuda.synchronize()
            want = depth_fit_rect_ref(dl, dr, *args, want, rect)
            assert st.cpu().numpy().tobytes() == want.tobytes(), (shape, name, step, st.cpu().numpy(), want)
        assert host.depth_fit_rect(dl, dr, *args, None, rect).tobytes() == depth_fit_rect_ref(dl, dr, *args, np.zeros(4, f32), rect).tobytes()
    a, b = torch.zeros(4, dtype=torch.float32, device="cuda"), torch.zeros(4, dtype=torch.float32, device="cuda")
    dev.d_depth_fit_rect(_cuda(dl), _cuda(dr), *args, a, None)
    dev.d_depth_fit(_cuda(dl), _cuda(dr), *args, b)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == depth_fit_ref(dl, dr, *args, np.zeros(4, f32)).tobytes()
    assert a.cpu().numpy().tobytes() != depth_fit_rect_ref(dl, dr, *args, np.zeros(4, f32), _rects(H, W)[3][1]).tobytes()


@pytest.mark.parametrize("shape", [(16, 17), (37, 61), (67, 130)], ids=lambda s: "%dx%d" % s)
def test_overlay_fit_rect(gpu_ready, shape):
    """every branch of the slide rule, per axis: intersecting, wholly above / left, wholly below / right, longer than the interval"""
    import torch
    from stm_amd import device_api as dev, host_api as host
    H, W = shape
    dl, dr = _pattern(H, W, 6), _pattern(H, W, 7)
    Hv, Wv = 2 * H, W + 5
    kw = dict(gain=0.75, conv=0.5, near_permille=20, margin=0.5, pad=1, limit_lo=-20.0, limit_hi=20.0, rate_near=1.0, rate_far=0.5)
    active = (H // 4, H - H // 4, W // 4, W - W // 4)
    ov_small = np.full((3, 4, 4), 255, np.uint8)
    ov_tall = np.full((Hv, 3, 4), 255, np.uint8)
    ov_wide = np.full((2, Wv, 4), 255, np.uint8)
    cases = [("inside", ov_small, Wv // 2, Hv // 2), ("crossing_top", ov_small, Wv // 2, 2 * active[0] - 2), ("above", ov_small, Wv // 2, 0),
             ("below", ov_small, Wv // 2, Hv - 3), ("left", ov_small, 0, Hv // 2), ("right", ov_small, Wv - 4, Hv // 2),
             ("corner", ov_small, Wv - 4, Hv - 3), ("taller", ov_tall, Wv // 2, 0), ("wider_in_the_bar", ov_wide, 0, Hv - 2)]
    results = set()
    for name, ov, x0, y0 in cases:
        st, want = torch.zeros(4, dtype=torch.float32, device="cuda"), None
        for step in range(2):
            dev.d_overlay_fit_rect(_cuda(dl), _cuda(dr), _cuda(ov), x0, y0, Hv, Wv, kw["limit_lo"], kw["limit_hi"], st, _rect(active),
                                   **{k: v for k, v in kw.items() if not k.startswith("limit")})
            torch.cuda.synchronize()
            want = overlay_fit_rect_ref(dl, dr, ov, x0, y0, Hv, Wv, active, state=want, **kw)
            assert st.cpu().numpy().tobytes() == want.tobytes(), (shape, name, step, st.cpu().numpy(), want)
        assert want[0] == 1
        assert host.overlay_fit_rect(dl, dr, ov, x0, y0, Hv, Wv, kw["limit_lo"], kw["limit_hi"], rect=active,
                                     **{k: v for k, v in kw.items() if not k.startswith("limit")}).tobytes() == \
            overlay_fit_rect_ref(dl, dr, ov, x0, y0, Hv, Wv, active, **kw).tobytes()
        results.add(want.tobytes())
    assert len(results) > 3
    a, b = torch.zeros(4, dtype=torch.float32, device="cuda"), torch.zeros(4, dtype=torch.float32, device="cuda")
    rest = {k: v for k, v in kw.items() if not k.startswith("limit")}
    dev.d_overlay_fit_rect(_cuda(dl), _cuda(dr), _cuda(ov_small), 0, 0, Hv, Wv, -20.0, 20.0, a, None, **rest)
    dev.d_overlay_fit(_cuda(dl), _cuda(dr), _cuda(ov_small), 0, 0, Hv, Wv, -20.0, 20.0, b, **rest)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == overlay_fit_ref(dl, dr, ov_small, 0, 0, Hv, Wv, **kw).tobytes()


# ------------------------------------------------------------------------------------------------------- 3. the frame calls
FH, FW = 64, 96
BARS = dict(top=8, bottom=8, left=0, right=12, level=0, noise=3)
BUDGET = (0.75, 0.5)            # depth mode 1: the frame of every run but the depth mode 2 one is rendered under it
AUTO = (-2.0, 2.0, 4.0, 20, 1.0)  # depth mode 2
OV_LIMITS = (-6.0, 6.0)
OV_AT = (20, 57)                # x0, y0: the strip lies wholly in the bottom bar
_PAIR = []


def _pair():
    """a synthetic pair whose picture is lit, inside noisy bars that are independent in the two eyes"""
    from stm_amd import synth
    if not _PAIR:
        L, R, _ = synth.stereo_pair(FH, FW, D, ZD, seed=77)
        L = np.clip(L.astype(np.int32) // 2 + 90, 0, 255).astype(np.uint8)
        R = np.clip(R.astype(np.int32) // 2 + 90, 0, 255).astype(np.uint8)
        L, R = paint_bars(L, seed=1, **BARS), paint_bars(R, seed=2, **BARS)
        P, Q, _ = synth.stereo_pair(FH, FW, D, ZD, seed=5)  # the history frame of the _t form
        for a in (L, R, P, Q):
            a.setflags(write=False)
        _PAIR.extend([L, R, np.ascontiguousarray(np.concatenate([P, Q], axis=1))])
    return _PAIR


def _params():
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=ZD, usd=17, lsd=8)


def _overlay():
    ov = np.zeros((6, 40, 4), np.uint8)
    ov[:, 4:36] = (40, 200, 250, 255)
    return ov


FORMS = ["stm", "t", "nv12", "2s", "half_linear"]
_HIST = {}


def _inputs(form):
    """(the call's input, packing, the unpacked pair as the call sees it)"""
    from stm_amd import synth
    L, R, _ = _pair()
    if form == "nv12":
        y, uv = synth.bgr_to_nv12(np.concatenate([L, R], axis=1), 0)
        return (y, uv), None, unpack_nv12_ref(y, uv, FH, FW, (0, 0, 0), 0, 0)
    if form == "half_linear":
        pk = (1, 0, 0, 0)
        f = synth.pack_frame(L, R, pk[0], pk[1], pk[3], fill=0x33)
        return f, pk, unpack_ref(f, FH, FW, pk[:3], pk[3])
    return np.ascontiguousarray(np.concatenate([L, R], axis=1)), None, (L, R)


def _call(form, inp, pk, stages=3):
    """one frame call of the form with the thread's settings as they are: (disp_l, disp_r, frame)"""
    import torch
    from stm_amd import device_api as dev
    p = _params()
    dl = torch.zeros((FH, FW), dtype=torch.float32, device="cuda")
    dr, out = torch.zeros_like(dl), torch.zeros((FH, FW, 3), dtype=torch.uint8, device="cuda")
    if pk is not None:
        dev.set_packing(*pk)
    try:
        if form == "nv12":
            dev.d_adcensus_stm_nv12(_cuda(inp[0]), _cuda(inp[1]), dl, dr, out, p, stages)
        elif form == "2s":
            dev.d_adcensus_stm_2s(_cuda(inp), dl, dr, out, p, FH // 2, FW // 2, 0.5, stages)
        elif form == "t":
            if not _HIST:  # the previous frame and its maps, from a call with every setting off
                prev = _pair()[2]
                hl = torch.zeros((FH, FW), dtype=torch.float32, device="cuda")
                hr, ho = torch.zeros_like(hl), torch.zeros((FH, FW, 3), dtype=torch.uint8, device="cuda")
                assert dev.get_active()[0] == 0, "the history is taken with the setting off"
                dev.d_adcensus_stm(_cuda(prev), hl, hr, ho, p, stages=2)
                torch.cuda.synchronize()
                _HIST["prev"] = (_cuda(prev), hl, hr)
            h = _HIST["prev"]
            dev.d_adcensus_stm_t(_cuda(inp), dl, dr, out, p, stages | 0x2000, h[0], h[1], h[2], 0.5, 765, 100.0)
        else:
            dev.d_adcensus_stm(_cuda(inp), dl, dr, out, p, stages=stages)
        torch.cuda.synchronize()
    finally:
        dev.set_packing(0, 0, 0, 0)
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


class _Thread:
    """the thread's settings for one run: depth mode 1 at BUDGET or mode 2 at AUTO, the active area, an automatic overlay"""

    def __init__(self, active=None, fill=None, depth_state=None, active_state=None, overlay=None, overlay_state=None, hold=1):
        self.active, self.fill, self.depth_state, self.active_state = active, fill, depth_state, active_state
        self.overlay, self.overlay_state, self.hold = overlay, overlay_state, hold

    def __enter__(self):
        from stm_amd import device_api as dev
        if self.depth_state is not None:
            dev.set_depth_auto(*AUTO, self.depth_state)
            dev.set_depth(2)
        else:
            dev.set_depth(1, *BUDGET)
        if self.overlay is not None:
            dev.set_overlay(self.overlay, OV_AT[0], OV_AT[1], 0.0)
            dev.set_overlay_auto(OV_LIMITS[0], OV_LIMITS[1], 20, 1.0, 0, 1.0, 0.1, self.overlay_state)
        fill = (False, 0.0) if self.fill is None else (True, self.fill)
        if self.active == "auto":
            dev.set_active_auto(24, 10, 300, self.hold, self.active_state)
            dev.set_active(2, None, *fill)
        elif self.active is not None:
            dev.set_active(1, self.active, *fill)
        return self

    def __exit__(self, *exc):
        from stm_amd import device_api as dev
        dev.set_active(0)
        dev.set_active_auto()
        dev.set_overlay_auto(None)
        dev.set_overlay(None)
        dev.set_depth(0)
        dev.set_depth_auto(-1.0, 1.0, 1.0, 20, 1.0, None)


def _render(orc, eyes, dl, dr, gain, conv):
    return render_depth_ref(render_chain(orc, eyes[0], eyes[1], dl, dr), 8, None, False, FH, FW, gain, conv)


@pytest.mark.parametrize("form", FORMS)
def test_frame_calls(gpu_ready, orc, form):
    import torch
    from stm_amd import device_api as dev
    inp, pk, eyes = _inputs(form)
    eyes = (np.ascontiguousarray(eyes[0][..., :3]), np.ascontiguousarray(eyes[1][..., :3]))
    want_state = detect_ref(eyes[0], None, 24, 10, 300, 1)[0]
    rect = rect_of(want_state)
    # (the linear expansion of a squeezed eye spreads the right bar's edge over one more column)
    assert rect == ((8, 56, 0, 85) if form == "half_linear" else (8, 56, 0, 84))
    with _Thread():
        off = _call(form, inp, pk)
    assert np.array_equal(off[2], _render(orc, eyes, off[0], off[1], *BUDGET)), form  # the yardstick itself holds with the setting off
    assert off[0].any() and off[2].any()

    # a given rectangle and a measured one, nothing reading them: the outputs are the call's with the setting off
    with _Thread(active=rect):
        got = _call(form, inp, pk)
    assert all(np.array_equal(a, b) for a, b in zip(got, off)), form
    state = _zero_state()
    with _Thread(active="auto", active_state=state):
        got = _call(form, inp, pk)
    assert all(np.array_equal(a, b) for a, b in zip(got, off)), form
    assert np.array_equal(state.cpu().numpy(), want_state), (form, state.cpu().numpy(), want_state)

    # fill: the maps are the off call's filled by hand, the frame is rendered from them; with a scratch state and with stages 2
    for active in (rect, "auto"):
        with _Thread(active=active, fill=-1.25):
            got = _call(form, inp, pk)
        d_l, d_r = _cuda(off[0]), _cuda(off[1])
        dev.d_active_fill(d_l, _rect(rect), -1.25)
        dev.d_active_fill(d_r, _rect(rect), -1.25)
        torch.cuda.synchronize()
        hand = (d_l.cpu().numpy(), d_r.cpu().numpy())
        assert hand[0].tobytes() == fill_ref(off[0], rect, -1.25).tobytes() and hand[1].tobytes() == fill_ref(off[1], rect, -1.25).tobytes()
        assert got[0].tobytes() == hand[0].tobytes() and got[1].tobytes() == hand[1].tobytes(), (form, active)
        assert np.array_equal(got[2], _render(orc, eyes, hand[0], hand[1], *BUDGET)), (form, active)
        assert not np.array_equal(got[0], off[0])
        filled = (hand[0], hand[1], got[2])
    if form in ("stm", "t", "nv12", "half_linear"):  # the full-resolution entries take a `stages` low byte below 3
        with _Thread():
            off2 = _call(form, inp, pk, stages=2)
        with _Thread(active="auto", fill=3.0):
            got2 = _call(form, inp, pk, stages=2)
        assert got2[0].tobytes() == fill_ref(off2[0], rect, 3.0).tobytes() and got2[1].tobytes() == fill_ref(off2[1], rect, 3.0).tobytes()

    # depth mode 2: the state is the fit under the rectangle by hand, the frame is rendered with it
    dstate = torch.zeros(4, dtype=torch.float32, device="cuda")
    with _Thread(active="auto", depth_state=dstate):
        got = _call(form, inp, pk)
    assert np.array_equal(got[0], off[0]) and np.array_equal(got[1], off[1])
    hand = torch.zeros(4, dtype=torch.float32, device="cuda")
    dev.d_depth_fit_rect(_cuda(off[0]), _cuda(off[1]), *AUTO, hand, _rect(rect))
    torch.cuda.synchronize()
    st = dstate.cpu().numpy()
    assert st.tobytes() == hand.cpu().numpy().tobytes() == depth_fit_rect_ref(off[0], off[1], *AUTO, np.zeros(4, f32), rect).tobytes(), form
    assert st.tobytes() != depth_fit_ref(off[0], off[1], *AUTO, np.zeros(4, f32)).tobytes()  # the bars would have moved it
    assert np.array_equal(got[2], _render(orc, eyes, off[0], off[1], st[1], st[2])), form

    # an automatic overlay wholly in the bottom bar, the maps filled: the state is the fit under the rectangle by hand on the filled
    # maps -- not the fill value, which is all the footprint itself holds -- and the frame is the filled call's with the overlay
    # composited by hand at the state's disparity
    ov = _overlay()
    d_ov, ostate = _cuda(ov), torch.zeros(4, dtype=torch.float32, device="cuda")
    with _Thread(active=rect, fill=-1.25, overlay=d_ov, overlay_state=ostate):
        got = _call(form, inp, pk)
    off = filled
    hand = torch.zeros(4, dtype=torch.float32, device="cuda")
    dev.d_overlay_fit_rect(_cuda(off[0]), _cuda(off[1]), d_ov, OV_AT[0], OV_AT[1], FH, FW, OV_LIMITS[0], OV_LIMITS[1], hand, _rect(rect),
                           gain=BUDGET[0], conv=BUDGET[1], near_permille=20, margin=1.0, pad=0, rate_near=1.0, rate_far=0.1)
    torch.cuda.synchronize()
    kw = dict(gain=BUDGET[0], conv=BUDGET[1], near_permille=20, margin=1.0, pad=0, limit_lo=OV_LIMITS[0], limit_hi=OV_LIMITS[1])
    st = ostate.cpu().numpy()
    assert st.tobytes() == hand.cpu().numpy().tobytes() == overlay_fit_rect_ref(off[0], off[1], ov, *OV_AT, FH, FW, rect, **kw).tobytes(), form
    assert float(overlay_fit_ref(off[0], off[1], ov, *OV_AT, FH, FW, **kw)[2]) == -1.25 * BUDGET[0] - BUDGET[1] != float(st[2])
    frame = _cuda(off[2])
    dev.d_mux_overlay(frame, d_ov, OV_AT[0], OV_AT[1], state_disparity_ref(st, *OV_LIMITS), 8)
    torch.cuda.synchronize()
    assert np.array_equal(got[2], frame.cpu().numpy()), form
    assert got[0].tobytes() == off[0].tobytes()


def off_outputs():
    """the frame calls of this file with the setting never set, or set and switched off again (the caller decides): a digest"""
    import hashlib
    h = hashlib.sha256()
    for form in FORMS:
        inp, pk, _ = _inputs(form)
        with _Thread():
            for o in _call(form, inp, pk):
                h.update(o.tobytes())
    return h.hexdigest()


def test_mode_0_is_a_process_that_never_set_the_area(gpu_ready):
    from stm_amd import device_api as dev
    state = _zero_state()
    dev.set_active_auto(24, 10, 300, 2, state)
    dev.set_active(2, None, True, 1.0)
    dev.set_active(1, (1, 9, 1, 9), True, 1.0)
    dev.set_active(0)
    dev.set_active_auto()
    here = off_outputs()
    assert (state == 0).all()
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_active as t\n"
            "print('digest', t.off_outputs())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ("digest " + here) in r.stdout, r.stdout + r.stderr


def test_host_flavour_frame(gpu_ready):
    """stm_adcensus_stm goes through the same body: the maps come back filled"""
    from stm_amd import device_api as dev, host_api as api
    L, R, _ = _pair()
    sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
    p = _params()
    args = (p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    plain = api.adcensus_stm(sbs, FW, FH, FW, *args)
    dev.set_active(2, None, True, -2.0)
    try:
        got = api.adcensus_stm(sbs, FW, FH, FW, *args)
    finally:
        dev.set_active(0)
    rect = rect_of(detect_ref(L, None, 24, 10, 300, 12)[0])
    assert got[0].tobytes() == fill_ref(plain[0], rect, -2.0).tobytes() and got[1].tobytes() == fill_ref(plain[1], rect, -2.0).tobytes()


def test_frame_rules(gpu_ready, lib):
    """a mode 1 rectangle that does not fit the frame is refused with nothing written; with the mode 0 the frame is taken"""
    import torch
    from stm_amd import device_api as dev
    lib.stm_set_error_mode(1)
    try:
        p = _params()
        H, W = 16, 32
        sbs = torch.zeros((H, 2 * W, 3), dtype=torch.uint8, device="cuda")
        dl = torch.full((H, W), 5.0, dtype=torch.float32, device="cuda")
        dr, out = torch.full_like(dl, 5.0), torch.full((H, W, 3), 0x77, dtype=torch.uint8, device="cuda")
        dev.set_active(1, (0, 17, 0, 32), True, 0.0)
        try:
            lib.stm_d_adcensus_stm(sbs.data_ptr(), dl.data_ptr(), dr.data_ptr(), out.data_ptr(), H, 2 * W, W, H, W, 3, p.num_views, p.angle,
                                   p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, 3)
            msg = lib.stm_last_error()
        finally:
            dev.set_active(0)
        torch.cuda.synchronize()
        assert b"d_adcensus_stm" in msg and b"rect" in msg, msg
        assert (dl == 5.0).all() and (out == 0x77).all()
    finally:
        lib.stm_set_error_mode(0)


# ------------------------------------------------------------------------------------------------------- 4. the frame stream
def _stream_frames():
    """8 frames at 48 x 96: shot A without bars (0 .. 2), with a 6-row letterbox from frame 3, a cut to shot B (6, 7) with 10-row bars"""
    from stm_amd import synth
    H, W = 48, 96
    A = [np.clip(x.astype(np.int32) // 2 + 90, 0, 255).astype(np.uint8) for x in synth.stereo_pair(H, W, D, ZD, seed=77)[:2]]
    B = [np.clip(x.astype(np.int32) // 4 + 190, 0, 255).astype(np.uint8) for x in synth.stereo_pair(H, W, 6, 1, seed=5)[:2]]
    frames = []
    for k in range(8):
        pair = A if k < 6 else B
        bar = 0 if k < 3 else (6 if k < 6 else 10)
        frames.append([paint_bars(e, top=bar, bottom=bar, level=0, noise=3, seed=10 * k + j) for j, e in enumerate(pair)])
    return H, W, frames


def stream_check():
    """.active() per frame against the numpy sequence (hold 2, the cut flag from the statement of the detector), the maps filled
    outside each frame's rectangle, and the setter's rules.  Returns a digest (the caller compares graphs on with graphs off)."""
    import hashlib
    from stm_amd import device_api as dev, video
    H, W, frames = _stream_frames()
    fs = video.FrameStream(H, W, _params(), cut=(370, 1), active_auto=(24, 10, 300, 2), active_fill=-1.5)
    outs, rects = [], []
    try:
        assert fs.active() is None  # -1 before a collect
        pending = 0
        for k, (L, R) in enumerate(frames):
            if pending == 2:
                outs.append(fs.collect())
                rects.append(fs.active())
                pending -= 1
            fs.submit(np.ascontiguousarray(np.concatenate([L, R], axis=1)))
            pending += 1
            if k == 0:  # the setter is refused after the first submit (as a return value: error mode 1)
                dev.lib().stm_set_error_mode(1)
                try:
                    with pytest.raises(ValueError, match="only before the first submit"):
                        fs.set_active(0)
                finally:
                    dev.lib().stm_set_error_mode(0)
        while pending:
            outs.append(fs.collect())
            rects.append(fs.active())
            pending -= 1
    finally:
        fs.close()
    cut, st, want, flags = None, None, [], []
    for L, _ in frames:
        cut = cut_ref(L, cut, 370, 1)
        st = detect_ref(L, st, 24, 10, 300, 2, cut_flag=int(cut[1]))[0]
        want.append(rect_of(st) + (int(st[5]),))
        flags.append(int(cut[1]))
    assert flags == [1, 0, 0, 0, 0, 0, 1, 0]
    assert [w[0] for w in want] == [0, 0, 0, 0, 6, 6, 10, 10]  # the bar of frame 3 is taken at frame 4 (hold 2), the cut's at once
    assert rects == want, (rects, want)
    h = hashlib.sha256()
    for k, o in enumerate(outs):
        assert o[0] == k
        t, b, l, r = want[k][:4]
        for m in (o[1], o[2]):
            assert (m[:t] == f32(-1.5)).all() and (m[b:] == f32(-1.5)).all() and not (m[t:b] == f32(-1.5)).all(), k
        for a in o[1:]:
            h.update(a.tobytes())
    return h.hexdigest()


def test_stream(gpu_ready):
    here = stream_check()
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_active as t\n"
            "print('digest', t.stream_check())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, STM_STREAM_GRAPH="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ("digest " + here) in r.stdout, r.stdout + r.stderr


def test_stream_rules_modes_0_and_1(gpu_ready, lib):
    from stm_amd import video
    H, W, frames = _stream_frames()
    sbs = [np.ascontiguousarray(np.concatenate(f, axis=1)) for f in frames[3:5]]
    lib.stm_set_error_mode(1)
    try:
        fs = video.FrameStream(H, W, _params())
        try:
            for bad in ((3, None), (1, None), (1, (0, H + 1, 0, W)), (1, (0, H, 0, W + 1)), (1, (5, 5, 0, W)), (2, None, 2), (2, None, 1, NAN),
                        (2, None, 0, 0.0, 255), (2, None, 0, 0.0, 24, 1000), (2, None, 0, 0.0, 24, 10, 451), (2, None, 0, 0.0, 24, 10, 300, 0)):
                with pytest.raises(ValueError):
                    fs.set_active(*bad)
            fs.set_active(2)
            fs.set_active(0)  # off again before the first submit
            off = []
            for f in sbs:
                fs.submit(f)
                off.append((fs.collect(), fs.active()))
        finally:
            fs.close()
        fs = video.FrameStream(H, W, _params(), active=(6, 42, 0, W), active_fill=2.0)
        try:
            one = []
            for f in sbs:
                fs.submit(f)
                one.append((fs.collect(), fs.active()))
        finally:
            fs.close()
    finally:
        lib.stm_set_error_mode(0)
    for k in range(2):
        assert off[k][1] == (0, H, 0, W, 0) and one[k][1] == (6, 42, 0, W, 0)
        for j in (1, 2):
            assert one[k][0][j].tobytes() == fill_ref(off[k][0][j], (6, 42, 0, W), 2.0).tobytes(), (k, j)


# ------------------------------------------------------------------------------------------------------- 5. the driver
def test_video_cli_prints_the_rectangles(gpu_ready, tmp_path):
    from stm_amd import bmp_io
    H, W, frames = _stream_frames()
    src = tmp_path / "in"
    src.mkdir()
    for k, (L, R) in enumerate(frames[:6]):
        bmp_io.write_bmp(str(src / ("f_%03d.bmp" % k)), np.ascontiguousarray(np.concatenate([L, R], axis=1)))
    args = [sys.executable, os.path.join(ROOT, "tools", "stm_video.py"), str(src), "8", "18.43", str(W), str(H), str(D), str(ZD),
            "10", "30", "6", "20", "17", "8", "20", "0.4", str(tmp_path / "o")]
    text = subprocess.check_output(args + ["--active-auto", "24", "10", "300", "2", "--active-fill", "0"]).decode()
    st = None
    for k, (L, _) in enumerate(frames[:6]):
        st = detect_ref(L, st, 24, 10, 300, 2)[0]
        assert "frame %d: active rows %d..%d cols %d..%d changed %d\n" % ((k,) + rect_of(st) + (int(st[5]),)) in text, (k, text)
    assert rect_of(st) == (6, 42, 0, W)
    assert subprocess.call(args + ["--active-auto", "24", "10"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0
