"""Overlay depth placement on the GPU (stm_overlay_fit / stm_d_overlay_fit, stm_set_overlay_auto, stm_stream_set_overlay_auto /
stm_stream_overlay_depth), bit for bit against the numpy statement of the definition (test_overlay_fit_ref) and the overlay's own
(test_overlay_ref): the stage on maps with NaNs, infinities and out-of-range values under overlays whose alpha box and footprint
take every shape, the frame calls against the same call with the setting and the overlay off, the frame stream against the same
frames as thread-level calls with one caller-owned state, the errors.  Every comparison is np.array_equal over the whole array, the
state's four floats as bits.  Every test leaves the thread's overlay, placement, layout, lens geometry, depth budget and detector
at mode 0."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_depth import AUTO, FILL, _arm, _clean, _frame, _params, _run, thread_depth
from test_gpu_lens import thread_lens
from test_gpu_overlay import HO, WO, H, N, W, _geometry, thread_overlay
from test_gpu_quilt import thread_layout
from test_lens_ref import LINEAR_WARP
from test_overlay_fit_ref import bits, overlay_fit_ref, state_disparity_ref, strip
from test_overlay_ref import PANEL, overlay_ref, random_overlay

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN, INF = float("nan"), float("inf")
# near_permille, margin, pad, limit_lo, limit_hi, rate_near, rate_far of the frame and stream tests: limits the fits of the 40 x 64
# synthetic frames (|delta| <= 8, views 72 / 64 as wide) reach on one side only, two different rates
FIT = dict(near_permille=20, margin=1.0, pad=3, limit_lo=-13.5, limit_hi=2.0, rate_near=1.0, rate_far=0.25)
# the stream's: the synthetic frames' near end is the same plane everywhere, so a percentile well inside the footprint's range makes
# the target move from overlay to overlay and both rates get used
STREAM_FIT = dict(FIT, near_permille=350, rate_near=0.75)


@contextlib.contextmanager
def thread_overlay_auto(state=None, **kw):
    """the calling thread's placement for the duration of the block; off again afterwards, whatever happens"""
    from stm_amd import device_api as dev
    try:
        dev.set_overlay_auto(state=state, **dict(FIT, **kw))
        yield
    finally:
        dev.set_overlay_auto(None)
        assert dev.get_overlay_auto()[0] == 0


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ----------------------------------------------------------------------------- 1. the stage
def _maps(Hm, Wm, seed):
    """quarter-pixel-ish values with NaN, +-inf and values beyond the bins' range sprinkled in, and a NaN block"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(2):
        m = (rng.randint(-60, 60, size=(Hm, Wm)) * 0.3125).astype(f32)
        at = rng.randint(0, Hm * Wm, 40)
        m.ravel()[at] = np.resize(np.array([NAN, INF, -INF, 3000.0, -3000.0, 511.9, -512.1, 1e30], f32), 40)
        m[3:6, 10:14] = NAN
        out.append(m)
    return out


def _stage_cases(Hv, Wv):
    """(overlay, x0, y0, pad): every alpha box and every footprint of the issue's list"""
    one = strip(5, 9, 4, 4, 2, 2)  # a one-pixel box inside a larger overlay
    edges = [strip(5, 9, 0, 3, 1, 3), strip(5, 9, 5, 8, 1, 3), strip(5, 9, 2, 6, 0, 1), strip(5, 9, 2, 6, 3, 4)]  # left, right, top, bottom
    whole = random_overlay(3, 5, 9)
    whole[0, 0, 3] = whole[4, 8, 3] = 255  # the box spans the whole overlay
    empty = np.zeros((5, 9, 4), np.uint8)
    empty[..., :3] = 7  # colour without alpha is still transparent
    cases = [(one, 6, 7, 0), (one, 6, 7, 2)] + [(e, 5, 6, 1) for e in edges] + [(whole, 3, 2, 0), (empty, 3, 2, 4)]
    cases += [(whole, -4, 5, 0), (whole, Wv - 3, 5, 1), (whole, 7, -2, 0), (whole, 7, Hv - 2, 2)]  # clipped on each side
    cases += [(whole, -9, 5, 0), (whole, Wv, 5, 0), (whole, 7, -5, 0), (whole, 7, Hv, 0)]  # empty footprints ...
    cases += [(whole, -12, 5, 3), (strip(5, 9, 0, 2), Wv - 1, 5, 0)]  # ... also with a pad that does not reach, and by the box alone
    cases += [(one, Wv // 2, Hv // 2, 4096), (random_overlay(4, Hv, Wv), 0, 0, 0)]  # the whole map: by the pad, by the overlay
    cases += [(strip(9, 60, 3, 43, 1, 7), 4, 9, 0)]  # 7 x 41 view pixels: the rectangle's run crosses the 256-pixel tile boundary
    return cases


VIEWS = [(44, 72), (66, 108), (77, 111), (22, 24)]  # the last: a tile of a 3 x 2 quilt of 44 x 72


@pytest.mark.parametrize("view", VIEWS, ids=["%dx%d" % v for v in VIEWS])
@pytest.mark.parametrize("size", [(44, 72), (50, 74)], ids=["44x72", "50x74"])
def test_stage_both_flavours(gpu_ready, size, view):
    """one state per flavour carried through the cases, so every fit after the first has a history; every third call restarts, and
    the device flavour sees a cut state whose flag is set on every fourth; near_permille 0, 20 and 499 in turn"""
    import torch
    from stm_amd import device_api as dev, host_api as api
    (Hm, Wm), (Hv, Wv) = size, view
    dl, dr = _maps(Hm, Wm, Hm + Hv)
    d_dl, d_dr = _cuda(dl), _cuda(dr)
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    try:
        _arm(lib)
        d_state = torch.zeros(4, dtype=torch.float32, device="cuda")
        want_d, want_h = np.zeros(4, f32), np.zeros(4, f32)
        cut = torch.zeros(260, dtype=torch.int32, device="cuda")
        moved = 0
        for k, (ov, x0, y0, pad) in enumerate(_stage_cases(Hv, Wv)):
            kw = dict(gain=(1.0, 0.5, 1.75)[k % 3], conv=(0.0, 2.0, -1.5)[k % 3], near_permille=(0, 20, 499)[k % 3], margin=(1.0, -0.5)[k & 1],
                      pad=pad, limit_lo=-20.5, limit_hi=11.25, rate_near=(1.0, 0.5)[k & 1], rate_far=0.125, restart=k % 3 == 2)
            flag = int(k % 4 == 3)
            cut[1] = flag
            d_ov = _cuda(ov)
            dev.d_overlay_fit(d_dl, d_dr, d_ov, x0, y0, Hv, Wv, state=d_state, cut_state=cut if k % 2 else None, **kw)
            new_d = overlay_fit_ref(dl, dr, ov, x0, y0, Hv, Wv, state=want_d, cut_flag=flag, **kw)
            assert bits(d_state.cpu().numpy()) == bits(new_d), ("device", k, d_state.cpu().numpy(), new_d)
            got = api.overlay_fit(dl, dr, ov, x0, y0, Hv, Wv, state=want_h, **kw)
            new_h = overlay_fit_ref(dl, dr, ov, x0, y0, Hv, Wv, state=want_h, **kw)
            assert bits(got) == bits(new_h), ("host", k, got, new_h)
            moved += int(bits(new_d) != bits(want_d))
            want_d, want_h = new_d, new_h
            assert np.array_equal(d_ov.cpu().numpy(), ov)  # read only
        assert moved >= 10  # the cases are not all empty footprints
        assert np.array_equal(d_dl.cpu().numpy(), dl, equal_nan=True) and np.array_equal(d_dr.cpu().numpy(), dr, equal_nan=True)
        assert _clean(lib)
    finally:
        lib.stm_set_error_mode(0)


def test_stage_all_nan_footprint_and_nan_state(gpu_ready):
    """an all-NaN footprint writes nothing; one number among the NaNs decides alone; a NaN in the old state goes to limit_lo"""
    import torch
    from stm_amd import device_api as dev
    dl, dr = np.full((44, 72), NAN, f32), np.full((44, 72), NAN, f32)
    ov = strip(5, 9, 0, 8)
    old = np.array([1, NAN, -0.0, 7], f32)
    d_state, d_ov = _cuda(old), _cuda(ov)
    kw = dict(near_permille=0, margin=0.0, pad=0, limit_lo=-7.0, limit_hi=30.0, rate_near=1.0, rate_far=1.0)
    dev.d_overlay_fit(_cuda(dl), _cuda(dr), d_ov, 3, 2, 44, 72, state=d_state, **kw)
    assert bits(d_state.cpu().numpy()) == bits(old)
    dr[4, 6] = 1.25
    dev.d_overlay_fit(_cuda(dl), _cuda(dr), d_ov, 3, 2, 44, 72, state=d_state, **kw)
    want = overlay_fit_ref(dl, dr, ov, 3, 2, 44, 72, state=old, **kw)
    assert bits(d_state.cpu().numpy()) == bits(want) == bits([1, -7, 1.25, 0])


def test_stage_alpha_box_beyond_one_block(gpu_ready):
    """the box kernel gives a block 2048 columns of every 512th row: a 530 x 2100 overlay takes two column chunks and a second row
    per block, with the box's four bounds set by pixels in different chunks and passes; then a fully opaque overlay of that size"""
    import torch
    from stm_amd import device_api as dev
    dl, dr = _maps(44, 72, 9)
    ov = np.zeros((530, 2100, 4), np.uint8)
    for r, q in ((3, 2050), (513, 2049), (300, 2047), (511, 2070)):  # box rows 3 .. 513, columns 2047 .. 2070
        ov[r, q] = (9, 9, 9, 200)
    kw = dict(near_permille=100, margin=0.5, pad=1, limit_lo=-40.0, limit_hi=40.0, rate_near=1.0, rate_far=1.0)
    for pixels, x0, y0 in ((ov, -2040, -490), (np.full((530, 2100, 4), 255, np.uint8), -2060, -500)):
        d_state = torch.zeros(4, dtype=torch.float32, device="cuda")
        dev.d_overlay_fit(_cuda(dl), _cuda(dr), _cuda(pixels), x0, y0, 44, 72, state=d_state, **kw)
        want = overlay_fit_ref(dl, dr, pixels, x0, y0, 44, 72, **kw)
        assert want[0] == 1 and bits(d_state.cpu().numpy()) == bits(want), (x0, y0, d_state.cpu().numpy(), want)


# ----------------------------------------------------------------------------- 2. the frame calls
def _overlays(Hv, Wv):
    """a strip whose text sits in its left third, and a small overlay that crosses the view's right and bottom borders"""
    a = np.zeros((6, Wv, 4), np.uint8)
    a[1:5, 2:Wv // 3] = random_overlay(11, 4, Wv // 3 - 2)
    a[1, 2, 3] = a[4, Wv // 3 - 1, 3] = 255
    return [(a, 0, Hv - 8), (random_overlay(12, 5, 9), Wv - 6, Hv - 3)]


def _check_frame(orc, run, elem_sz=3, lens=None, layout=None, budget=(1.0, 0.0)):
    """run() -> (dl, dr, out).  With the thread's overlay and placement on: the maps are those of the same call with both off, the
    caller's state is overlay_fit_ref's on those maps (two calls: the second has a history), and the frame is overlay_ref of the
    plain call's at the state's disparity.  budget: (gain, conv), or a callable that returns the pair after a call (depth mode 2)."""
    import torch
    shift, coords, (Hv, Wv) = _geometry(orc, HO, WO, elem_sz, lens, layout)
    dl, dr, base = run()
    for ov, x0, y0 in _overlays(Hv, Wv):
        d_ov = _cuda(ov)
        state = torch.zeros(4, dtype=torch.float32, device="cuda")
        want_st = np.zeros(4, f32)
        for step in range(2):
            with thread_overlay(d_ov, x0, y0, 99.0), thread_overlay_auto(state):  # the setter's disparity is ignored
                dl2, dr2, out = run()
            g, c = budget() if callable(budget) else budget
            assert np.array_equal(dl2, dl) and np.array_equal(dr2, dr)
            want_st = overlay_fit_ref(dl2, dr2, ov, x0, y0, Hv, Wv, gain=g, conv=c, state=want_st, **FIT)
            assert bits(state.cpu().numpy()) == bits(want_st), (x0, y0, step, state.cpu().numpy(), want_st)
            want = overlay_ref(base, ov, x0, y0, state_disparity_ref(want_st, FIT["limit_lo"], FIT["limit_hi"]), shift, coords)
            assert not np.array_equal(want, base)
            assert np.array_equal(out, want), (x0, y0, step, int((out != want).sum()))
            state[1] = 40.0  # far behind: the second call comes nearer at rate_near, from a value outside the limits
            want_st[1] = 40.0
        assert want_st[0] == 1 and np.array_equal(d_ov.cpu().numpy(), ov)
    # no state of the caller's: scratch memory, every frame on its own
    ov, x0, y0 = _overlays(Hv, Wv)[0]
    with thread_overlay(_cuda(ov), x0, y0, 0.0), thread_overlay_auto(None):
        dl2, dr2, out = run()
    g, c = budget() if callable(budget) else budget
    st = overlay_fit_ref(dl2, dr2, ov, x0, y0, Hv, Wv, gain=g, conv=c, **FIT)
    assert np.array_equal(out, overlay_ref(base, ov, x0, y0, state_disparity_ref(st, FIT["limit_lo"], FIT["limit_hi"]), shift, coords))


@pytest.mark.parametrize("case", ["plain", "plain_4_byte_pixels", "0x800", "lens3", "depth1", "depth2", "depth2_null_state", "quilt_area",
                                  "agg_variant_200"])
def test_frame_device_flavour(gpu_ready, orc, case):
    import torch
    from stm_amd import device_api as dev
    sbs, p = _frame(H, W), _params(N)
    elem_sz = 4 if case == "plain_4_byte_pixels" else 3
    stages = 3 | (LINEAR_WARP if case == "0x800" else 0)
    lens = (3,) + PANEL if case == "lens3" else None
    layout = (1, 4, 2, 3) if case == "quilt_area" else None
    budget = (1.0, 0.0)
    lo, hi, mg, clip = AUTO
    with contextlib.ExitStack() as stack:
        if lens:
            stack.enter_context(thread_lens(*lens))
        if layout:
            stack.enter_context(thread_layout(4, 2, 3, 1))
        if case == "depth1":
            stack.enter_context(thread_depth(1, 0.6, 1.5))
            budget = (0.6, 1.5)
        if case.startswith("depth2"):
            dstate = torch.zeros(4, dtype=torch.float32, device="cuda") if case == "depth2" else None
            dev.set_depth_auto(lo, hi, mg, clip, 0.5, dstate)  # a carried state: every call of the test moves it
            stack.enter_context(thread_depth(2))
        try:
            dev.lib().stm_set_agg_variant(200 if case == "agg_variant_200" else 0)
            run = lambda: _run(sbs, p, stages, HO, WO, elem_sz)
            if case == "depth2":
                # the renderer of the plain call must see the same budget as the call under test: both start from the same state
                def run():
                    dstate.copy_(torch.tensor([1.0, 0.75, 0.5, 0.0]))
                    return _run(sbs, p, stages, HO, WO, elem_sz)
                budget = lambda: tuple(float(v) for v in dstate.cpu().numpy()[1:3])
            if case == "depth2_null_state":
                from test_depth_ref import depth_fit_ref
                dl0, dr0, _ = run()
                st = depth_fit_ref(dl0, dr0, lo, hi, mg, clip, 0.5, np.zeros(4, f32))
                budget = (float(st[1]), float(st[2]))
            _check_frame(orc, run, elem_sz, lens, layout, budget)
        finally:
            dev.lib().stm_set_agg_variant(0)
            dev.lib().stm_set_depth_auto(-1.0, 1.0, 1.0, 20, 1.0, None)


def test_frame_reduced_2s(gpu_ready, orc):
    import torch
    from stm_amd import device_api as dev
    sbs, p = _frame(H, W, 3), _params(N)

    def run():
        dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        dr = torch.zeros_like(dl)
        out = torch.full((HO, WO, 3), FILL, dtype=torch.uint8, device="cuda")
        dev.d_adcensus_stm_2s(_cuda(np.array(sbs)), dl, dr, out, p, 20, 32, 0.5, 3 | 0x1000)
        torch.cuda.synchronize()
        return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()
    _check_frame(orc, run)


def test_frame_nv12_input(gpu_ready, orc):
    import torch
    from stm_amd import device_api as dev, synth
    sbs, p = _frame(H, W, 7), _params(N)
    y, uv = synth.bgr_to_nv12(sbs, 1)

    def run():
        dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        dr = torch.zeros_like(dl)
        out = torch.full((HO, WO, 3), FILL, dtype=torch.uint8, device="cuda")
        dev.d_adcensus_stm_nv12(_cuda(np.array(y)), _cuda(np.array(uv)), dl, dr, out, p, 3, matrix=1)
        torch.cuda.synchronize()
        return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()
    _check_frame(orc, run)


def test_frame_host_flavour(gpu_ready, orc):
    """stm_adcensus_stm, which ends in the device flavour's tail: overlay and state stay device memory"""
    from stm_amd import host_api as api
    sbs, p = _frame(H, W), _params(N)
    args = (p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    _check_frame(orc, lambda: api.adcensus_stm(np.array(sbs), W, HO, WO, *args))


def test_a_cut_restarts_the_fit(gpu_ready, orc):
    """the detector on over the shots A, A, B: the third frame's state is a fresh fit of its maps, the second's is not"""
    import torch
    from stm_amd import device_api as dev
    from test_gpu_cut import THRESH, _shot
    Hc, Wc = 48, 96
    p = dev.FrameParams(num_disp=16, zero_disp=8, usd=17, lsd=8)
    shots = {k: np.ascontiguousarray(np.concatenate(_shot(Hc, Wc, k), axis=1)) for k in "AB"}
    ov, x0, y0 = strip(6, 40, 2, 30, 1, 4), 20, 36
    state = torch.zeros(4, dtype=torch.float32, device="cuda")
    cstate = torch.zeros(260, dtype=torch.int32, device="cuda")
    kw = dict(FIT, rate_near=0.5, rate_far=0.5, limit_lo=-30.0, limit_hi=30.0)
    want = np.zeros(4, f32)
    flags, fresh, wants = [], [], []
    try:
        dev.set_cut(1, THRESH, 1, cstate)
        with thread_overlay(_cuda(ov), x0, y0, 0.0), thread_overlay_auto(state, **dict(rate_near=0.5, rate_far=0.5, limit_lo=-30.0, limit_hi=30.0)):
            for k in "AAB":
                dl, dr, _ = _run(shots[k], p, 3)
                flag = int(cstate.cpu().numpy()[1])
                flags.append(flag)
                fresh.append(overlay_fit_ref(dl, dr, ov, x0, y0, Hc, Wc, **kw))
                want = overlay_fit_ref(dl, dr, ov, x0, y0, Hc, Wc, state=want, cut_flag=flag, **kw)
                assert bits(state.cpu().numpy()) == bits(want), (k, state.cpu().numpy(), want)
                wants.append(want.copy())
                if len(flags) == 1:
                    state[1] = 25.0  # a history the second frame must follow at rate 0.5, not drop
                    want[1] = 25.0
    finally:
        dev.set_cut(0)
    assert flags == [1, 0, 1]
    assert bits(wants[2]) == bits(fresh[2]) and bits(wants[1]) != bits(fresh[1])


# ----------------------------------------------------------------------------- 3. the frame stream
def _schedule():
    """frame -> the overlay in force when it is submitted: (pixels, x0, y0) or None.  Size, place and presence change"""
    A, B = random_overlay(21, 6, 20), strip(9, 31, 3, 22, 2, 6)
    a0, b0, b1, a1 = (A, 4, 3), (B, -5, 15), (B, 30, 30), (A, 12, -2)
    return [a0, a0, b0, b1, None, a1, a1, a1]


def _stream_run(p, frames, stages, schedule, auto, **kw):
    """the frames through a FrameStream, two in flight; stm_stream_overlay is called only where the overlay changes.  Returns
    [(index, dl, dr, out, overlay_depth)]"""
    from stm_amd import video
    fs = video.FrameStream(H, W, p, HO, WO, stages=stages, overlay=(16, 40), overlay_auto=auto, **kw)
    got = []
    try:
        for k, f in enumerate(frames):
            if k >= 2:
                got.append(fs.collect() + (fs.overlay_depth(),))
            if k == 0 or schedule[k] is not schedule[k - 1]:
                if schedule[k] is None:
                    fs.overlay(None)
                else:
                    fs.overlay(np.array(schedule[k][0]), schedule[k][1], schedule[k][2], 77.0)  # its disparity is ignored
            assert fs.submit(f) == k
        got.append(fs.collect() + (fs.overlay_depth(),))
        got.append(fs.collect() + (fs.overlay_depth(),))
    finally:
        fs.close()
    assert [g[0] for g in got] == list(range(len(frames)))
    return got


def _thread_run(p, frames, stages, schedule, depth_auto):
    """the same eight frames as thread-level frame calls with one caller-owned state; a new overlay zeroes `valid`"""
    import torch
    from stm_amd import device_api as dev
    state = torch.zeros(4, dtype=torch.float32, device="cuda")
    dstate = torch.zeros(4, dtype=torch.float32, device="cuda")
    got, prev = [], None
    with contextlib.ExitStack() as stack:
        if depth_auto:
            dev.set_depth_auto(*depth_auto, dstate)
            stack.enter_context(thread_depth(2))
        try:
            for k, f in enumerate(frames):
                d_sbs = _cuda(np.array(f))
                dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
                dr = torch.zeros_like(dl)
                out = torch.zeros((HO, WO, 3), dtype=torch.uint8, device="cuda")
                with contextlib.ExitStack() as inner:
                    if schedule[k] is not None:
                        if k == 0 or schedule[k] is not schedule[k - 1]:
                            state[0] = 0  # restart
                        inner.enter_context(thread_overlay(_cuda(schedule[k][0]), schedule[k][1], schedule[k][2], 0.0))
                        inner.enter_context(thread_overlay_auto(state, **STREAM_FIT))
                    if stages & 0x2000:
                        dev.d_adcensus_stm_t(d_sbs, dl, dr, out, p, stages, *(prev if prev else (None, None, None)))
                    else:
                        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=stages)
                    torch.cuda.synchronize()
                prev = (d_sbs, dl, dr)
                got.append((k, dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy(), state.cpu().numpy()))
        finally:
            dev.lib().stm_set_depth_auto(-1.0, 1.0, 1.0, 20, 1.0, None)
    return got


@pytest.mark.parametrize("case", ["graphs", "no_graphs", "temporal_0x2000", "depth2"])
def test_stream_equals_the_thread_level_calls(gpu_ready, monkeypatch, case):
    """8 frames: both slots replay their captured graphs (from their second frame on) while overlay, place and presence change; the
    frames, the maps and stm_stream_overlay_depth are those of the thread-level calls; the thread's own settings never reach the
    stream and are not changed by it"""
    import torch
    from stm_amd import device_api as dev
    if case == "no_graphs":
        monkeypatch.setenv("STM_STREAM_GRAPH", "0")
    stages = 3 | (0x2000 if case == "temporal_0x2000" else 0)
    lo, hi, mg, clip = AUTO
    depth_auto = (lo, hi, mg, clip, 0.5) if case == "depth2" else None
    p = _params(N)
    frames = [_frame(H, W, 40 + (k % 3)) for k in range(8)]
    schedule = _schedule()
    auto = tuple(STREAM_FIT[n] for n in ("limit_lo", "limit_hi", "near_permille", "margin", "pad", "rate_near", "rate_far"))
    want = _thread_run(p, frames, stages, schedule, depth_auto)
    mine = _cuda(random_overlay(23, 4, 4))
    with thread_overlay(mine, 1, 1, 3.0), thread_overlay_auto(None, limit_lo=-1.0, limit_hi=1.0):
        got = _stream_run(p, frames, stages, schedule, auto, depth_auto=depth_auto)
        assert dev.get_overlay() == (1, 4, 4, 1, 1, 3.0) and dev.get_overlay_auto()[4:6] == (-1.0, 1.0)
    disparities = set()
    for k in range(8):
        assert np.array_equal(got[k][1], want[k][1]) and np.array_equal(got[k][2], want[k][2]), k
        assert bits(got[k][4]) == bits(want[k][4]), (k, got[k][4], want[k][4])
        assert np.array_equal(got[k][3], want[k][3]), (k, int((got[k][3] != want[k][3]).sum()))
        disparities.add(float(got[k][4][1]))
    assert got[7][4][0] == 1 and len(disparities) >= 2  # the state moved


def test_refusals(gpu_ready):
    import torch
    from stm_amd import device_api as dev, video
    lib = dev.lib()
    p = _params(N)
    lib.stm_set_error_mode(1)
    try:
        # the stage: nothing written
        state = _cuda(np.array([1, 5, 6, 7], f32))
        dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        ov = _cuda(random_overlay(1, 3, 5))
        for kw, word in ((dict(near_permille=500), "near_permille"), (dict(pad=-1), "pad"), (dict(limit_lo=3.0, limit_hi=2.0), "limit_lo"),
                         (dict(rate_far=0.0), "rate_far"), (dict(gain=-1.0), "gain"), (dict(margin=NAN), "margin")):
            _arm(lib)
            dev.d_overlay_fit(dl, dl.clone(), ov, 0, 0, HO, WO, **dict(dict(limit_lo=-5.0, limit_hi=5.0, state=state), **kw))
            assert word.encode() in lib.stm_last_error(), kw
        assert bits(state.cpu().numpy()) == bits([1, 5, 6, 7])
        # the thread's setter
        with pytest.raises(ValueError, match="rate_near"):
            dev.set_overlay_auto(-5.0, 5.0, rate_near=1.5)
        assert dev.get_overlay_auto()[0] == 0
        # the stream: before stm_stream_set_overlay, bad parameters, after the first submit
        fs = video.FrameStream(H, W, p, HO, WO)
        try:
            with pytest.raises(ValueError, match="stm_stream_set_overlay"):
                fs.set_overlay_auto(1, -5.0, 5.0)
            fs.set_overlay(6, 20)
            with pytest.raises(ValueError, match="mode"):
                fs.set_overlay_auto(2, -5.0, 5.0)
            with pytest.raises(ValueError, match="limit_lo"):
                fs.set_overlay_auto(1, 5.0, -5.0)
            with pytest.raises(ValueError, match="pad"):
                fs.set_overlay_auto(1, -5.0, 5.0, pad=5000)
            fs.set_overlay_auto(1, -5.0, 5.0)
            fs.set_overlay(0, 0)  # the overlay off: the placement goes with it
            fs.set_overlay(6, 20)
            assert fs.overlay_depth() is None  # nothing collected yet
            fs.overlay(random_overlay(1, 6, 20), 2, 3, 1.0)
            assert fs.submit(_frame(H, W)) == 0
            with pytest.raises(ValueError, match="first submit"):
                fs.set_overlay_auto(1, -5.0, 5.0)
            fs.collect()
            assert bits(fs.overlay_depth()) == bits([0, 1, 0, 0])  # the placement off: the disparity the frame was submitted under
        finally:
            fs.close()
    finally:
        lib.stm_set_error_mode(0)
    assert dev.get_overlay()[0] == 0 and dev.get_overlay_auto()[0] == 0


# ----------------------------------------------------------------------------- 4. mode 0
def off_outputs():
    """frame calls with an overlay on and the placement never set or set to mode 0 (the caller decides): a digest of the outputs"""
    import hashlib
    h = hashlib.sha256()
    sbs, p = _frame(H, W), _params(N)
    with thread_overlay(_cuda(random_overlay(11, 6, 20)), -3, 2, 2.5):
        for stages in (3, 3 | LINEAR_WARP):
            for o in _run(sbs, p, stages, HO, WO):
                h.update(o.tobytes())
    for o in _run(sbs, p, 3, HO, WO):
        h.update(o.tobytes())
    return h.hexdigest()


def test_mode_0_is_a_process_that_never_touched_the_setting(gpu_ready):
    import torch
    from stm_amd import device_api as dev
    state = torch.zeros(4, dtype=torch.float32, device="cuda")
    dev.set_overlay_auto(-5.0, 5.0, state=state)
    dev.set_overlay_auto(None)
    here = off_outputs()
    assert (state == 0).all()
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_overlay_fit as t\n"
            "print('digest', t.off_outputs())\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ("digest " + here) in r.stdout, r.stdout + r.stderr
