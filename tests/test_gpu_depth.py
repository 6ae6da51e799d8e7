"""Depth budget control on the GPU (stm_set_depth, stm_set_depth_auto, stm_depth_fit / stm_d_depth_fit, the frame stream's three
calls), bit for bit against the numpy statement of the definitions (test_depth_ref) on the oracle's chain -- the four floats of the
state included.  Every test leaves the thread's depth budget and lens geometry at mode 0."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_depth_ref import depth_fit_ref, render_depth_ref
from test_lens_ref import INTERP, LINEAR_WARP, SUBPIXEL, frame_chain, render_chain

pytestmark = pytest.mark.gpu

f32 = np.float32
T = 0x2000
GUIDED = 0x1000
PANEL = (7.37, 0.86, 0.3)
PANEL_B = (5.5, -1.25, -0.4)
FILL = 0x5A
NAN, INF = float("nan"), float("inf")
# disp_lo, disp_hi, max_gain, clip_permille.  The 40 x 64 frames of seeds 30 and 31 span [-4, 3.75] and [-4, -1.25] after the clip
# (the oracle's maps), so this budget gives them the gains 0.4516 and 1.2727: neither 1 nor max_gain, and not the same
AUTO = (-1.5, 2.0, 1.5, 20)


def _arm(lib):
    """plant a known message (error mode 1): a later check sees the call's own message or this one, never an earlier test's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


def _clean(lib):
    return b"d_filter_median" in lib.stm_last_error()


@contextlib.contextmanager
def thread_depth(mode, gain=1.0, conv=0.0, lens=None):
    """the calling thread's depth budget (and lens geometry) for the duration of the block; both off again afterwards"""
    from stm_amd import device_api as dev
    try:
        if lens is not None:
            dev.set_lens(*lens)
        dev.set_depth(mode, gain, conv)
        yield
    finally:
        assert dev.lib().stm_set_depth(0, 0.0, 0.0) == 0
        assert dev.lib().stm_set_lens(0, 0.0, 0.0, 0.0) == 0


def _params(N=8, D=16, zd=8, usd=17, lsd=8):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd, num_views=N)


_FRAMES = {}


def _frame(H, W, seed_off=0, D=16, zd=8):
    from stm_amd import synth
    key = (H, W, seed_off, D, zd)
    if key not in _FRAMES:
        sbs = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + seed_off)[0]
        sbs.setflags(write=False)
        _FRAMES[key] = sbs
    return _FRAMES[key]


def _pad(sbs, elem_sz):
    if elem_sz == 3:
        return np.array(sbs)
    return np.concatenate([sbs, np.full(sbs.shape[:2] + (elem_sz - 3,), 0xC3, np.uint8)], axis=2)


def _run(sbs, p, stages, Ho=None, Wo=None, elem_sz=3):
    import torch
    from stm_amd import device_api as dev
    H, W = sbs.shape[0], sbs.shape[1] // 2
    d_sbs = torch.from_numpy(_pad(sbs, elem_sz)).cuda()
    dl = torch.full((H, W), float(FILL), dtype=torch.float32, device="cuda")
    dr = torch.full_like(dl, float(FILL))
    out = torch.full((Ho or H, Wo or W, elem_sz), FILL, dtype=torch.uint8, device="cuda")
    dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _chain_of(orc, sbs, dl, dr):
    """the renderer's planes from the maps a call returned (pinned to the oracle by the tests of the stages that made them)"""
    L, R = orc.demux_sbs(np.array(sbs), sbs.shape[1] // 2)
    return render_chain(orc, L, R, dl, dr)


# ----------------------------------------------------------------------------- 1. the fit as a stage
FIT_SHAPES = [(1, 1), (3, 5), (7, 257), (33, 1023), (64, 64)]


def _fit_maps(kind, H, W, seed):
    rng = np.random.RandomState(seed)
    if kind == "random":
        return [(rng.randint(-60, 61, size=(H, W)) * 0.25).astype(f32) for _ in range(2)]
    if kind == "edges":  # exactly on the x.125 bin edges, both signs
        return [((rng.randint(-40, 41, size=(H, W)) * 2 + 1) * 0.125).astype(f32) for _ in range(2)]
    if kind == "constant":
        return [np.full((H, W), 2.25, f32), np.full((H, W), 2.25, f32)]
    assert kind == "special"
    maps = [(rng.randint(-60, 61, size=(H, W)) * 0.25).astype(f32) for _ in range(2)]
    vals = [NAN, INF, -INF, 1e9, -1e9]
    for m in maps:
        flat = m.reshape(-1)
        for i, v in enumerate(vals):
            flat[(i * 7) % flat.size] = v
    return maps


@pytest.mark.parametrize("kind", ["random", "edges", "constant", "special"])
@pytest.mark.parametrize("shape", FIT_SHAPES, ids=["%dx%d" % s for s in FIT_SHAPES])
def test_depth_fit_both_flavours(gpu_ready, shape, kind):
    """stm_depth_fit and stm_d_depth_fit: the state after the call is the statement's, bit for bit, from valid = 0 and from a valid
    state with rate 0.25, for several clips; the maps are read only"""
    import torch
    from stm_amd import device_api as dev, host_api as api
    H, W = shape
    dl, dr = _fit_maps(kind, H, W, 17 * H + W)
    keep = dl.copy(), dr.copy()
    t_l, t_r = torch.from_numpy(dl).cuda(), torch.from_numpy(dr).cuda()
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    try:
        _arm(lib)
        for lo, hi, mg, clip in ((-4.0, 4.0, 1.0, 0), (-1.5, 2.0, 3.0, 20), (-0.7, 0.3, 8.0, 499)):
            for state, rate in ((np.zeros(4, f32), 1.0), (np.array([1, 0.75, -1.25, 0], f32), 0.25), (np.array([0, 5, 5, 5], f32), 0.25)):
                want = depth_fit_ref(dl, dr, lo, hi, mg, clip, rate, state)
                got = api.depth_fit(dl, dr, lo, hi, mg, clip, rate, state)
                assert got.tobytes() == want.tobytes(), ("host", lo, hi, mg, clip, rate, got, want)
                st = torch.from_numpy(state.copy()).cuda()
                dev.d_depth_fit(t_l, t_r, lo, hi, mg, clip, rate, st)
                torch.cuda.synchronize()
                assert st.cpu().numpy().tobytes() == want.tobytes(), ("device", lo, hi, mg, clip, rate, st.cpu().numpy(), want)
        assert _clean(lib)
    finally:
        lib.stm_set_error_mode(0)
    for a, b, t in zip(keep, (dl, dr), (t_l, t_r)):
        assert a.tobytes() == b.tobytes() == t.cpu().numpy().tobytes()


# ----------------------------------------------------------------------------- 2. frames against the statement
SETTINGS = [(1.0, 0.0), (0.5, 0.0), (0.0, 2.0), (1.5, -3.25), (1.0, None)]  # None: conv = 2 W, which exercises the clamp
LENSES = [None, (1,) + PANEL, (2,) + PANEL_B, (3,) + PANEL]
SIZES = [((32, 64), (40, 64)), ((37, 53), (50, 81))]


def _frame_case(orc, sizes, elem_sz, N, stages):
    from stm_amd import device_api as dev
    (H, W), (Ho, Wo) = sizes
    sbs, p = _frame(H, W), _params(N)
    extra = stages & ~0xff
    ch = frame_chain(orc, sbs, p, extra)
    linear = bool(extra & LINEAR_WARP)
    lib = dev.lib()
    before = _run(sbs, p, stages, Ho, Wo, elem_sz)
    assert np.array_equal(before[0], ch["dl"]) and np.array_equal(before[1], ch["dr"])
    seen = set()
    try:
        for lens in LENSES:
            for gain, conv in SETTINGS:
                conv = 2.0 * W if conv is None else conv
                want = render_depth_ref(ch, N, lens, linear, Ho, Wo, gain, conv, p.angle, elem_sz)
                with thread_depth(1, gain, conv, lens):
                    dl, dr, out = _run(sbs, p, stages, Ho, Wo, elem_sz)
                    if (gain, conv) == (1.5, -3.25):  # the un-fused variant has no views to write either: same bytes
                        lib.stm_set_agg_variant(200)
                        unfused = _run(sbs, p, stages, Ho, Wo, elem_sz)[2]
                        lib.stm_set_agg_variant(0)
                        assert np.array_equal(unfused, out), (lens, gain, conv)
                assert np.array_equal(dl, ch["dl"]) and np.array_equal(dr, ch["dr"]), (lens, gain, conv)
                assert np.array_equal(out[..., :3], want), (lens, gain, conv, int((out[..., :3] != want).sum()))
                assert (out[..., 3:] == FILL).all()
                seen.add(out.tobytes())
    finally:
        lib.stm_set_agg_variant(0)
    assert len(seen) == len(LENSES) * len(SETTINGS)  # every setting shows
    after = _run(sbs, p, stages, Ho, Wo, elem_sz)  # mode 0 again: today's bytes
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert before[2].tobytes() not in seen


@pytest.mark.parametrize("stages", [3, 3 | LINEAR_WARP], ids=["0x3", "0x803"])
@pytest.mark.parametrize("N", [8, 5])
@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("sizes", SIZES, ids=["32x64_to_40x64", "37x53_to_50x81"])
def test_frame_against_the_statement(gpu_ready, orc, sizes, elem_sz, N, stages):
    """stm_d_adcensus_stm in depth mode 1: five (gain, conv) pairs under the reference's view assignment and lens modes 1, 2 and 3;
    the maps are untouched, stm_set_agg_variant(200) gives the same bytes, and with mode 0 again the call gives today's output"""
    _frame_case(orc, sizes, elem_sz, N, stages)


def test_frame_with_subpixel_and_interpolated_maps(gpu_ready, orc):
    _frame_case(orc, SIZES[1], 3, 8, 3 | SUBPIXEL | INTERP)


# ----------------------------------------------------------------------------- 3. mode 2
def test_automatic_mode_fits_renders_and_keeps_its_state(gpu_ready, orc):
    """the maps the call returns go through the statement's fit, then through its render; the caller's d_state is the statement's
    state, a second call at rate 0.5 continues from it, zeroing `valid` restarts; a null d_state fits every frame on its own"""
    import torch
    from stm_amd import device_api as dev
    H, W, Ho, Wo = 40, 64, 50, 81
    p = _params(8)
    frames = [_frame(H, W, k) for k in (30, 31)]
    lib = dev.lib()
    lo, hi, mg, clip = AUTO
    state = torch.zeros(4, dtype=torch.float32, device="cuda")
    want_st = np.zeros(4, f32)
    gains = []
    lib.stm_set_error_mode(1)
    try:
        _arm(lib)
        for step, (k, rate, lens, stages) in enumerate(((0, 1.0, None, 3), (1, 0.5, (3,) + PANEL, 3 | LINEAR_WARP), (0, 0.5, (2,) + PANEL_B, 3),
                                                        (1, 0.5, None, 3))):
            if step == 3:
                state[0] = 0  # a scene cut: the history restarts
                want_st[0] = 0
            dev.set_depth_auto(lo, hi, mg, clip, rate, state)
            with thread_depth(2, lens=lens):
                dl, dr, out = _run(frames[k], p, stages, Ho, Wo)
            ch = _chain_of(orc, frames[k], dl, dr)
            want_st = depth_fit_ref(dl, dr, lo, hi, mg, clip, rate, want_st)
            assert state.cpu().numpy().tobytes() == want_st.tobytes(), (step, state.cpu().numpy(), want_st)
            want = render_depth_ref(ch, 8, lens, bool(stages & LINEAR_WARP), Ho, Wo, want_st[1], want_st[2])
            assert np.array_equal(out, want), step
            gains.append(float(want_st[1]))
        assert want_st[0] == 1 and len(set(gains)) == 4 and gains[0] < 1 < gains[3] < mg, gains  # fits that neither bound decides
        # no state of the caller's: scratch memory, every frame on its own whatever the rate
        dev.set_depth_auto(lo, hi, mg, clip, 0.25, None)
        for k in (0, 1):
            with thread_depth(2):
                dl, dr, out = _run(frames[k], p, 3, Ho, Wo)
            st = depth_fit_ref(dl, dr, lo, hi, mg, clip, 0.25, np.zeros(4, f32))
            assert np.array_equal(out, render_depth_ref(_chain_of(orc, frames[k], dl, dr), 8, None, False, Ho, Wo, st[1], st[2])), k
        assert state.cpu().numpy().tobytes() == want_st.tobytes()
        assert _clean(lib)
    finally:
        lib.stm_set_error_mode(0)
        lib.stm_set_depth(0, 0.0, 0.0)
        lib.stm_set_depth_auto(-1.0, 1.0, 1.0, 20, 1.0, None)  # drop the pointer to this test's tensor


# ----------------------------------------------------------------------------- 4. the other frame calls
def test_nv12_frame(gpu_ready, orc):
    import torch
    from stm_amd import device_api as dev, synth
    from test_nv12_ref import nv12_to_bgr_ref
    H, W = 40, 64
    sbs, p = _frame(H, W, 7), _params(8)
    y, uv = synth.bgr_to_nv12(sbs, 1)
    bgr = np.ascontiguousarray(nv12_to_bgr_ref(y, uv, 1))
    ch = frame_chain(orc, bgr, p, LINEAR_WARP)
    dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    with thread_depth(1, 0.75, 1.5, (3,) + PANEL):
        dev.d_adcensus_stm_nv12(torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(np.array(uv)).cuda(), dl, dr, out, p,
                                3 | LINEAR_WARP, matrix=1)
        torch.cuda.synchronize()
    assert np.array_equal(dl.cpu().numpy(), ch["dl"]) and np.array_equal(dr.cpu().numpy(), ch["dr"])
    assert np.array_equal(out.cpu().numpy(), render_depth_ref(ch, 8, (3,) + PANEL, True, H, W, 0.75, 1.5))


def test_temporal_frame_fits_the_stabilised_maps(gpu_ready, orc):
    """stm_d_adcensus_stm_t with a history, mode 2: the fit sees the maps the call returns, which are the stabilised ones"""
    import torch
    from stm_amd import device_api as dev
    H, W = 40, 64
    p = _params(8)
    a, b = _frame(H, W, 0), _frame(H, W, 1)
    lo, hi, mg, clip = AUTO
    dla, dra, _ = _run(a, p, 3)
    d_b = torch.from_numpy(np.array(b)).cuda()
    hist = [torch.from_numpy(np.array(x)).cuda() for x in (a, dla, dra)]
    outs = {}
    for stages in (3, 3 | T):
        dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        dr = torch.zeros_like(dl)
        out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        dev.set_depth_auto(lo, hi, mg, clip, 1.0, None)
        with thread_depth(2):
            dev.d_adcensus_stm_t(d_b, dl, dr, out, p, stages, hist[0], hist[1], hist[2], 0.5, 765, 100.0)
            torch.cuda.synchronize()
        dl, dr = dl.cpu().numpy(), dr.cpu().numpy()
        st = depth_fit_ref(dl, dr, lo, hi, mg, clip, 1.0, np.zeros(4, f32))
        assert np.array_equal(out.cpu().numpy(), render_depth_ref(_chain_of(orc, b, dl, dr), 8, None, False, H, W, st[1], st[2])), stages
        outs[stages] = (dl, out.cpu().numpy())
    assert not np.array_equal(outs[3][0], outs[3 | T][0])  # the wide gates did blend the maps


def test_reduced_frame_fits_the_upscaled_maps(gpu_ready, orc):
    """stm_d_adcensus_stm_2s with 0x1000, mode 2: the fit sees the guided up-scaled maps the call returns"""
    import torch
    from stm_amd import device_api as dev
    H, W, h, w, scale, Ho, Wo = 40, 64, 20, 32, 0.5, 50, 81
    sbs, p = _frame(H, W, 3), _params(8)
    lo, hi, mg, clip = AUTO
    dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros((Ho, Wo, 3), dtype=torch.uint8, device="cuda")
    dev.set_depth_auto(lo, hi, mg, clip, 1.0, None)
    with thread_depth(2, lens=(1,) + PANEL):
        dev.d_adcensus_stm_2s(torch.from_numpy(np.array(sbs)).cuda(), dl, dr, out, p, h, w, scale, 3 | GUIDED)
        torch.cuda.synchronize()
    dl, dr = dl.cpu().numpy(), dr.cpu().numpy()
    st = depth_fit_ref(dl, dr, lo, hi, mg, clip, 1.0, np.zeros(4, f32))
    assert np.array_equal(out.cpu().numpy(), render_depth_ref(_chain_of(orc, sbs, dl, dr), 8, (1,) + PANEL, False, Ho, Wo, st[1], st[2]))


def test_host_flavour(gpu_ready, orc):
    """stm_adcensus_stm, which ends in the device flavour's render"""
    from stm_amd import host_api as api
    H, W, Ho, Wo = 37, 53, 50, 81
    sbs, p = _frame(H, W), _params(8)
    ch = frame_chain(orc, sbs, p, 0)
    args = (p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    plain = api.adcensus_stm(np.array(sbs), W, Ho, Wo, *args)
    with thread_depth(1, 0.6, -1.75):
        dl, dr, out = api.adcensus_stm(np.array(sbs), W, Ho, Wo, *args)
    assert np.array_equal(dl, ch["dl"]) and np.array_equal(dr, ch["dr"])
    assert np.array_equal(out, render_depth_ref(ch, 8, None, False, Ho, Wo, 0.6, -1.75))
    for a, b in zip(plain, api.adcensus_stm(np.array(sbs), W, Ho, Wo, *args)):  # mode 0 again
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- 5. the frame stream
def test_stream_manual_mode_is_the_frame_call(gpu_ready):
    """three frames (the third is captured and replayed) equal the per-frame call; setters after the first submit return -1; a
    thread-level stm_set_depth made while the stream runs neither reaches the stream nor is changed by it"""
    from stm_amd import device_api as dev, video
    H, W = 40, 64
    p = _params(8)
    frames = [_frame(H, W, 20 + k) for k in range(3)]
    lib = dev.lib()
    fs = video.FrameStream(H, W, p, stages=3 | LINEAR_WARP, lens=(3,) + PANEL, depth=(0.5, 1.25))
    lib.stm_set_error_mode(1)
    got = []
    try:
        assert fs.depth() is None
        assert fs.submit(frames[0]) == 0
        assert lib.stm_stream_set_depth(fs._h, 1, 1.0, 0.0) == -1 and b"first submit" in lib.stm_last_error()
        assert lib.stm_stream_set_depth_auto(fs._h, -1.0, 1.0, 1.0, 20, 1.0) == -1 and b"first submit" in lib.stm_last_error()
        assert lib.stm_set_depth(1, 2.0, -4.0) == 0  # the thread's budget changes under the stream
        assert fs.submit(frames[1]) == 1
        got.append(fs.collect())
        assert fs.depth() == (0.5, 1.25)
        assert fs.submit(frames[2]) == 2
        got.append(fs.collect())
        got.append(fs.collect())
        thread_out = _run(frames[0], p, 3)[2]  # the submits put the thread's own setting back
    finally:
        lib.stm_set_error_mode(0)
        lib.stm_set_depth(0, 0.0, 0.0)
        fs.close()
    with thread_depth(1, 2.0, -4.0):
        assert np.array_equal(_run(frames[0], p, 3)[2], thread_out)
    assert not np.array_equal(_run(frames[0], p, 3)[2], thread_out)
    with thread_depth(1, 0.5, 1.25, (3,) + PANEL):
        for k, f in enumerate(frames):
            dl, dr, out = _run(f, p, 3 | LINEAR_WARP)
            assert got[k][0] == k and np.array_equal(got[k][1], dl) and np.array_equal(got[k][2], dr), k
            assert np.array_equal(got[k][3], out), k


def stream_auto_check(temporal):
    """automatic mode at rate 0.25 over six frames of two alternating inputs (the later frames replay the slots' graphs, unless
    STM_STREAM_GRAPH=0): stm_stream_depth follows the statement's recursion on the maps each frame returns, and every interlaced
    frame is the statement's render at that state"""
    from oracle import pyoracle as orc
    from stm_amd import device_api as dev, video
    orc.build()
    H, W = 40, 64
    p = _params(8)
    inputs = [_frame(H, W, 30), _frame(H, W, 31)]
    lo, hi, mg, clip = AUTO
    stages = 3 | (T if temporal else 0)
    lib = dev.lib()
    fs = video.FrameStream(H, W, p, stages=stages, depth_auto=(lo, hi, mg, clip, 0.25))
    got, applied = [], []
    try:
        assert lib.stm_set_depth(1, 2.0, -4.0) == 0  # the thread's own budget: must not reach the stream
        pending = 0
        for k in range(6):
            if pending == 2:
                got.append(fs.collect())
                applied.append(fs.depth())
                pending -= 1
            assert fs.submit(inputs[k & 1]) == k
            pending += 1
        while pending:
            got.append(fs.collect())
            applied.append(fs.depth())
            pending -= 1
    finally:
        lib.stm_set_depth(0, 0.0, 0.0)
        fs.close()
    st = np.zeros(4, f32)
    gains = []
    for k in range(6):
        idx, dl, dr, out = got[k]
        assert idx == k
        st = depth_fit_ref(dl, dr, lo, hi, mg, clip, 0.25, st)
        assert (f32(applied[k][0]), f32(applied[k][1])) == (st[1], st[2]), (k, applied[k], st)
        want = render_depth_ref(_chain_of(orc, inputs[k & 1], dl, dr), 8, None, False, H, W, st[1], st[2])
        assert np.array_equal(out, want), (k, int((out != want).sum()))
        gains.append(float(st[1]))
    assert len(set(gains)) > 1  # the two inputs' fits differ, so the state moved
    if not temporal:
        for k in range(2, 6):
            assert np.array_equal(got[k][1], got[k - 2][1])  # the maps of a frame depend on its input alone


@pytest.mark.parametrize("temporal", [False, True], ids=["plain", "temporal"])
def test_stream_automatic_mode(gpu_ready, temporal):
    stream_auto_check(temporal)


def test_stream_automatic_mode_without_graphs_in_a_child_process(gpu_ready):
    """STM_STREAM_GRAPH is read when the stream is created, so a child process (as the existing overlap test starts its children)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_depth as t\n"
            "t.stream_auto_check(True)\n"
            "print('ok')\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, STM_STREAM_GRAPH="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ----------------------------------------------------------------------------- 6. errors
BAD_DEPTH = [(3, 1.0, 0.0, b"mode"), (-1, 1.0, 0.0, b"mode"), (1, NAN, 0.0, b"gain"), (1, -0.125, 0.0, b"gain"), (1, 8.5, 0.0, b"gain"),
             (1, INF, 0.0, b"gain"), (1, 1.0, NAN, b"conv"), (1, 1.0, INF, b"conv"), (1, 1.0, -4097.0, b"conv")]
BAD_AUTO = [(1.0, 1.0, 1.0, 20, 1.0, b"disp_lo"), (2.0, 1.0, 1.0, 20, 1.0, b"disp_lo"), (NAN, 1.0, 1.0, 20, 1.0, b"disp_lo"),
            (-1.0, INF, 1.0, 20, 1.0, b"disp_hi"), (-4097.0, 1.0, 1.0, 20, 1.0, b"disp_lo"), (-1.0, 1.0, 0.0, 20, 1.0, b"max_gain"),
            (-1.0, 1.0, 8.5, 20, 1.0, b"max_gain"), (-1.0, 1.0, NAN, 20, 1.0, b"max_gain"), (-1.0, 1.0, 1.0, -1, 1.0, b"clip_permille"),
            (-1.0, 1.0, 1.0, 500, 1.0, b"clip_permille"), (-1.0, 1.0, 1.0, 20, 0.0, b"rate"), (-1.0, 1.0, 1.0, 20, 1.5, b"rate"),
            (-1.0, 1.0, 1.0, 20, NAN, b"rate")]


def test_setters_refuse_bad_arguments_and_keep_the_old_setting(gpu_ready, orc):
    import torch
    from stm_amd import device_api as dev, video
    H, W = 32, 64
    sbs, p = _frame(H, W), _params(8)
    ch = frame_chain(orc, sbs, p, 0)
    lib = dev.lib()
    fs = video.FrameStream(H, W, p)
    state = torch.zeros(4, dtype=torch.float32, device="cuda")
    lo, hi, mg, clip = AUTO
    lib.stm_set_error_mode(1)
    try:
        assert lib.stm_stream_set_depth(fs._h, 2, 0.0, 0.0) == -1 and b"stream_set_depth_auto" in lib.stm_last_error()  # no budget yet
        assert lib.stm_set_depth(1, 0.5, 1.25) == 0
        for mode, gain, conv, word in BAD_DEPTH:
            _arm(lib)
            assert lib.stm_set_depth(mode, gain, conv) == -1
            err = lib.stm_last_error()
            assert b"set_depth" in err and word in err, err
            assert lib.stm_stream_set_depth(fs._h, mode, gain, conv) == -1
            err = lib.stm_last_error()
            assert b"stream_set_depth" in err and word in err, err
        with pytest.raises(ValueError):
            dev.set_depth(1, 9.0, 0.0)
        with pytest.raises(ValueError):
            fs.set_depth(1, 1.0, 5000.0)
        assert np.array_equal(_run(sbs, p, 3)[2], render_depth_ref(ch, 8, None, False, H, W, 0.5, 1.25))  # still the last accepted pair
        assert lib.stm_set_depth(0, NAN, INF) == 0  # mode 0: the other arguments are ignored
        dev.set_depth_auto(lo, hi, mg, clip, 1.0, state)
        for a in BAD_AUTO:
            _arm(lib)
            assert lib.stm_set_depth_auto(*a[:5], None) == -1
            err = lib.stm_last_error()
            assert b"set_depth_auto" in err and a[5] in err, err
            assert lib.stm_stream_set_depth_auto(fs._h, *a[:5]) == -1
            err = lib.stm_last_error()
            assert b"stream_set_depth_auto" in err and a[5] in err, err
        with pytest.raises(ValueError):
            dev.set_depth_auto(1.0, -1.0)
        _arm(lib)
        with thread_depth(2):  # still the last accepted parameters, the caller's state included
            dl, dr, out = _run(sbs, p, 3)
        st = depth_fit_ref(dl, dr, lo, hi, mg, clip, 1.0, np.zeros(4, f32))
        assert state.cpu().numpy().tobytes() == st.tobytes()
        assert np.array_equal(out, render_depth_ref(ch, 8, None, False, H, W, st[1], st[2]))
        assert _clean(lib)
    finally:
        lib.stm_set_error_mode(0)
        lib.stm_set_depth(0, 0.0, 0.0)
        lib.stm_set_depth_auto(-1.0, 1.0, 1.0, 20, 1.0, None)
        fs.close()


def test_fit_errors_write_nothing(gpu_ready):
    """every argument rule of stm_depth_fit / stm_d_depth_fit: reported before anything is launched or written"""
    import torch
    from stm_amd import device_api as dev
    lib = dev.lib()
    H, W = 3, 5
    f32p = C.POINTER(C.c_float)
    maps = np.zeros((2, H, W), f32)
    h_state = np.full(4, 7.5, f32)
    d_maps = torch.zeros((2, H, W), dtype=torch.float32, device="cuda")
    d_state = torch.full((4,), 7.5, dtype=torch.float32, device="cuda")
    cases = [(H, W) + a for a in BAD_AUTO] + [(0, W, -1.0, 1.0, 1.0, 20, 1.0, b"num_rows"), (H, 0, -1.0, 1.0, 1.0, 20, 1.0, b"num_cols"),
                                            (65536, 32768, -1.0, 1.0, 1.0, 20, 1.0, b"2^31")]
    dev._use_current_stream()
    lib.stm_set_error_mode(1)
    try:
        for rows, cols, lo, hi, mg, clip, rate, word in cases:
            _arm(lib)
            lib.stm_depth_fit(maps[0].ctypes.data_as(f32p), maps[1].ctypes.data_as(f32p), rows, cols, lo, hi, mg, clip, rate,
                              h_state.ctypes.data_as(f32p))
            err = lib.stm_last_error()
            assert b"depth_fit" in err and b"d_depth_fit" not in err and word in err, err
            lib.stm_d_depth_fit(dev._p(d_maps[0]), dev._p(d_maps[1]), rows, cols, lo, hi, mg, clip, rate, dev._p(d_state))
            torch.cuda.synchronize()
            err = lib.stm_last_error()
            assert b"d_depth_fit" in err and word in err, err
    finally:
        lib.stm_set_error_mode(0)
    assert (h_state == 7.5).all() and (d_state.cpu().numpy() == 7.5).all()
