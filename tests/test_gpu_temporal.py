"""Temporal disparity stabilisation on the GPU (stm_disp_temporal / stm_d_disp_temporal, the frame with a history
stm_d_adcensus_stm_t and its bit 0x2000, the frame stream with that bit), every comparison bit for bit against the numpy
statement of the definition (test_temporal_ref)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_temporal_ref import (ALPHA, HSLO, INTERP, KNOWN_IDS, LINEAR_WARP, SEQ, SHAPE_IDS, SHAPES, SUBPIXEL, TEMPORAL, THRESH_COLOR,
                               THRESH_DISP, halves, known_cases, mixed_sequence, render_ref, sad_max, temporal_case,
                               temporal_recursion, temporal_ref)

pytestmark = pytest.mark.gpu

_REF = {}


def _case(shape, elem_sz):
    """One random case per shape and pixel size with its reference, computed once and shared read-only"""
    key = (shape, elem_sz)
    if key not in _REF:
        H, W = shape
        arrays = temporal_case(H * 13 + W + elem_sz, H, W, elem_sz)
        want = temporal_ref(*arrays)
        for a in arrays + (want,):
            a.setflags(write=False)
        _REF[key] = arrays + (want,)
    return _REF[key]


def _both_flavours(cur, prev, img, img_prev, alpha, tc, td, want):
    """host_api.disp_temporal and device_api.d_disp_temporal against `want`; the inputs are read only"""
    import torch
    from stm_amd import device_api as dev, host_api as api
    keep = [np.array(a) for a in (cur, prev, img, img_prev)]
    got = api.disp_temporal(cur, prev, img, img_prev, alpha, tc, td)
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True), "host"
    t = [torch.from_numpy(np.array(a)).cuda() for a in (cur, prev, img, img_prev)]
    dev.d_disp_temporal(*t, alpha, tc, td)
    torch.cuda.synchronize()
    assert np.array_equal(t[0].cpu().numpy(), want, equal_nan=True), "device"
    for a, b, x in zip(keep[1:], (prev, img, img_prev), t[1:]):
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, x.cpu().numpy(), equal_nan=True)
    assert np.array_equal(keep[0], cur, equal_nan=True)


def _arm(lib):
    """stm_last_error keeps a thread's last message until its next failure.  Plant a known one (error mode 1 only), so that a
    check after the call under test sees either that call's own message or this one, never an earlier test's."""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


def _no_new_error(lib):
    return b"d_filter_median" in lib.stm_last_error()


# ----------------------------------------------------------------------------- 1. per stage
@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("name", KNOWN_IDS)
def test_temporal_known_answers(gpu_ready, name, elem_sz):
    case = [c for c in known_cases(elem_sz) if c[0] == name][0]
    _both_flavours(*case[1:])


@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_temporal_random_cases(gpu_ready, shape, elem_sz):
    """image pairs on both sides of the colour gate, maps on both sides of the disparity gate with NaN and +-inf in either"""
    cur, prev, img, img_prev, want = _case(shape, elem_sz)
    H, W = shape
    if H * W >= 300:
        m = sad_max(img, img_prev)
        assert (m <= THRESH_COLOR).any() and (m > THRESH_COLOR).any()
        assert np.isnan(cur).any() and np.isinf(prev).any() and not np.array_equal(want, cur, equal_nan=True)
    _both_flavours(cur, prev, img, img_prev, ALPHA, THRESH_COLOR, THRESH_DISP, want)


@pytest.mark.parametrize("params", [(0.25, 9, float("inf")), (1.0, 40, 0.0), (0.0, 765, 2.0), (0.75, 0, 1.0)],
                         ids=["inf_gate", "alpha_1_exact_gate", "alpha_0", "static_only"])
def test_temporal_other_parameters(gpu_ready, params):
    cur, prev, img, img_prev, _ = _case(SHAPES[3], 3)
    _both_flavours(cur, prev, img, img_prev, *params, temporal_ref(cur, prev, img, img_prev, *params))


def test_temporal_scattered_unaligned_buffers(gpu_ready, stm):
    """every buffer carved from one arena at an odd / 4-byte-only aligned address (4-byte pixels that are no aligned dwords
    included); the margins stay untouched"""
    import torch
    from test_gpu_caller_buffers import Arena, P, read
    lib = stm.lib()
    lib.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for elem_sz in (3, 4):
        cur, prev, img, img_prev, want = _case(SHAPES[3], elem_sz)
        H, W = SHAPES[3]
        arena = Arena(True, nbytes=1 << 20)
        d_img, d_cur, d_ip, d_prev = arena.put(img, 3), arena.put(cur, 12), arena.put(img_prev, 5), arena.put(prev, 4)
        lib.stm_d_disp_temporal(P(d_cur), P(d_prev), P(d_img), P(d_ip), H, W, elem_sz, ALPHA, THRESH_COLOR, THRESH_DISP)
        assert arena.intact()
        assert np.array_equal(read(d_cur, np.float32, (H, W)), want, equal_nan=True)
        assert np.array_equal(read(d_img, np.uint8, img.shape), img) and np.array_equal(read(d_ip, np.uint8, img.shape), img_prev)
        assert np.array_equal(read(d_prev, np.float32, (H, W)), prev, equal_nan=True)


def test_temporal_argument_errors(gpu_ready, stm):
    """each is reported with the call's name and the argument's, and the caller's map is left unwritten"""
    import torch
    lib = stm.lib()
    u8p, f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    img = np.full((4, 6, 3), 7, np.uint8)
    cur = np.full((4, 6), 7, np.float32)
    prev = np.full((4, 6), 8, np.float32)
    pc, pq, pi = cur.ctypes.data_as(f32p), prev.ctypes.data_as(f32p), img.ctypes.data_as(u8p)
    d_cur = torch.full((4, 6), 7.0, dtype=torch.float32, device="cuda")
    d_prev = torch.full((4, 6), 8.0, dtype=torch.float32, device="cuda")
    d_img = torch.full((4, 6, 3), 7, dtype=torch.uint8, device="cuda")
    nan, inf = float("nan"), float("inf")
    bad = [((4, 6, 2, 0.5, 24, 1.5), b"elem_sz"), ((0, 6, 3, 0.5, 24, 1.5), b"num_rows"), ((4, 0, 3, 0.5, 24, 1.5), b"num_cols"),
           ((4, 6, 3, -0.01, 24, 1.5), b"alpha"), ((4, 6, 3, 1.01, 24, 1.5), b"alpha"), ((4, 6, 3, nan, 24, 1.5), b"alpha"),
           ((4, 6, 3, inf, 24, 1.5), b"alpha"), ((4, 6, 3, 0.5, -1, 1.5), b"thresh_color"), ((4, 6, 3, 0.5, 766, 1.5), b"thresh_color"),
           ((4, 6, 3, 0.5, 24, -0.5), b"thresh_disp"), ((4, 6, 3, 0.5, 24, nan), b"thresh_disp"), ((4, 6, 3, 0.5, 24, -inf), b"thresh_disp")]
    lib.stm_set_error_mode(1)
    try:
        for args, word in bad:
            _arm(lib)
            lib.stm_disp_temporal(pc, pq, pi, pi, *args)
            err = lib.stm_last_error()
            assert err and word in err and b"disp_temporal" in err and b"d_disp_temporal" not in err, (args, err)
            _arm(lib)
            lib.stm_d_disp_temporal(d_cur.data_ptr(), d_prev.data_ptr(), d_img.data_ptr(), d_img.data_ptr(), *args)
            err = lib.stm_last_error()
            assert err and word in err and b"d_disp_temporal" in err, (args, err)
        # prev must not alias cur
        _arm(lib)
        lib.stm_disp_temporal(pc, pc, pi, pi, 4, 6, 3, 0.5, 24, 1.5)
        err = lib.stm_last_error()
        assert err and b"alias" in err and b"disp_temporal" in err, err
        _arm(lib)
        lib.stm_d_disp_temporal(d_cur.data_ptr(), d_cur.data_ptr() + 16, d_img.data_ptr(), d_img.data_ptr(), 4, 6, 3, 0.5, 24, 1.5)
        err = lib.stm_last_error()
        assert err and b"alias" in err and b"d_disp_temporal" in err, err
        # the limits themselves are legal
        for args in ((4, 6, 3, 0.0, 0, 0.0), (4, 6, 3, 1.0, 765, inf)):
            _arm(lib)
            lib.stm_d_disp_temporal(d_cur.data_ptr(), d_prev.data_ptr(), d_img.data_ptr(), d_img.data_ptr(), *args)
            torch.cuda.synchronize()
            assert _no_new_error(lib), args
            d_cur.fill_(7.0)
    finally:
        lib.stm_set_error_mode(0)
    torch.cuda.synchronize()
    assert np.all(cur == 7) and bool((d_cur == 7).all()) and bool((d_prev == 8).all())


# ----------------------------------------------------------------------------- 2. the frame
def _params():
    from stm_amd import device_api as dev
    s = SEQ
    return dev.FrameParams(num_disp=s["D"], zero_disp=s["zd"], usd=s["usd"], lsd=s["lsd"])


def _run(sbs, p, stages, fill=0):
    """stm_d_adcensus_stm on buffers pre-filled with `fill`"""
    import torch
    from stm_amd import device_api as dev
    H, W = sbs.shape[0], sbs.shape[1] // 2
    d_sbs = torch.from_numpy(np.array(sbs)).cuda()
    dl = torch.full((H, W), float(fill), dtype=torch.float32, device="cuda")
    dr = torch.full_like(dl, float(fill))
    out = torch.full((H, W, 3), fill, dtype=torch.uint8, device="cuda")
    dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _run_t(sbs, p, stages, hist=None, params=(ALPHA, THRESH_COLOR, THRESH_DISP), fill=0):
    """stm_d_adcensus_stm_t on buffers pre-filled with `fill`; hist = (previous sbs, previous disp_l, previous disp_r) or None"""
    import torch
    from stm_amd import device_api as dev
    H, W = sbs.shape[0], sbs.shape[1] // 2
    d_sbs = torch.from_numpy(np.array(sbs)).cuda()
    dl = torch.full((H, W), float(fill), dtype=torch.float32, device="cuda")
    dr = torch.full_like(dl, float(fill))
    out = torch.full((H, W, 3), fill, dtype=torch.uint8, device="cuda")
    h = [None, None, None] if hist is None else [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in hist]
    dev.d_adcensus_stm_t(d_sbs, dl, dr, out, p, stages, h[0], h[1], h[2], *params)
    torch.cuda.synchronize()
    if hist is not None:  # the history is read only
        for a, t in zip(hist, h):
            assert a is None or np.array_equal(a, t.cpu().numpy(), equal_nan=True)
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _recursion_t(frames, p, stages, params=(ALPHA, THRESH_COLOR, THRESH_DISP)):
    """the frames of a sequence through stm_d_adcensus_stm_t, each with the frame before it as its history"""
    got = []
    for k, f in enumerate(frames):
        got.append(_run_t(f, p, stages, None if k == 0 else (frames[k - 1], got[-1][0], got[-1][1]), params))
    return got


_FRAMES = {}


def _sequence(n):
    if n not in _FRAMES:
        _FRAMES[n] = mixed_sequence(n)
        for f in _FRAMES[n]:
            f.setflags(write=False)
    return _FRAMES[n]


T = TEMPORAL
STAGE_WORDS = [2 | T, 3 | T, 3 | T | INTERP, 3 | T | SUBPIXEL | LINEAR_WARP, 3 | T | HSLO]


@pytest.mark.parametrize("stages", STAGE_WORDS, ids=["0x%x" % s for s in STAGE_WORDS])
def test_frame_with_history_vs_chain(gpu_ready, orc, stages):
    """40 x 72, D = 8, three consecutive frames: the maps are the device frame's without the bit followed by temporal_ref applied
    recursively, the interlaced frame is the oracle chain rendering from those maps"""
    p = _params()
    frames = _sequence(3)
    plain = [_run(f, p, 2 | (stages & ~0xff & ~T & ~LINEAR_WARP))[:2] for f in frames]
    want = temporal_recursion(frames, plain)
    got = _recursion_t(frames, p, stages)
    changed = False
    for k, f in enumerate(frames):
        assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]), k
        changed |= k > 0 and not np.array_equal(want[k][0], plain[k][0])
        if (stages & 0xff) == 3:
            L, R = halves(f)
            mux = render_ref(orc, L, R, want[k][0], want[k][1], p, linear=bool(stages & LINEAR_WARP))
            assert np.array_equal(got[k][2], mux), k
        else:
            assert not got[k][2].any()  # stages 2 renders nothing
    assert changed  # the step did something
    for k in (1, 2):  # ... and left alone what moved
        for v in (0, 1):
            moved = sad_max(halves(frames[k])[v], halves(frames[k - 1])[v]) > THRESH_COLOR
            assert moved.any() and np.array_equal(got[k][v][moved], plain[k][v][moved])


def test_frame_with_other_parameters(gpu_ready):
    p = _params()
    frames = _sequence(3)
    params = (0.25, 30, 0.75)
    plain = [_run(f, p, 2)[:2] for f in frames]
    want = temporal_recursion(frames, plain, *params)
    got = _recursion_t(frames, p, 2 | T, params)
    for k in range(3):
        assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]), k
    assert not np.array_equal(want[2][0], temporal_recursion(frames, plain)[2][0])


@pytest.mark.parametrize("side", ["left", "right"])
def test_seam_of_the_halves(gpu_ready, side):
    """One half changes strongly in the column next to the seam while the other half is static: the static view is filtered in
    every pixel, its column at the seam included (the history maps are the frame's own maps + 1, so every pixel that is
    filtered moves by about 0.5), and the two columns of the other view next to the seam are left alone"""
    p = _params()
    H, W = SEQ["H"], SEQ["W"]
    f0 = _sequence(3)[0]
    f1 = np.array(f0)
    col = W if side == "left" else W - 1
    f1[:, col] = (f1[:, col].astype(np.int32) + 128) % 256
    static = 0 if side == "left" else 1
    base = _run(f1, p, 2)[:2]
    hist = (f0, base[0] + np.float32(1), base[1] + np.float32(1))
    got = _run_t(f1, p, 2 | T, hist)
    want = [temporal_ref(base[v], hist[1 + v], halves(f1)[v], halves(f0)[v]) for v in (0, 1)]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not sad_max(halves(f1)[static], halves(f0)[static]).any()
    assert (got[static] != base[static]).all()  # every pixel of the static view moved, the seam column included
    edge = 0 if static == 0 else W - 1
    moved = got[1 - static]
    assert np.array_equal(moved[:, [0, 1] if edge == 0 else [W - 2, W - 1]], base[1 - static][:, [0, 1] if edge == 0 else [W - 2, W - 1]])


def test_null_history_is_the_plain_frame(gpu_ready):
    p = _params()
    f = _sequence(3)[1]
    for bits in (0, SUBPIXEL | LINEAR_WARP):
        a, b = _run_t(f, p, 3 | T | bits, None), _run(f, p, 3 | bits)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # without the bit the history is ignored
    a = _run_t(f, p, 3, (_sequence(3)[0], np.zeros((SEQ["H"], SEQ["W"]), np.float32), np.zeros((SEQ["H"], SEQ["W"]), np.float32)))
    assert all(np.array_equal(x, y) for x, y in zip(a, _run(f, p, 3)))


def test_frame_errors(gpu_ready):
    """every error is reported through stm_last_error before anything is launched: the buffers keep their fill value"""
    import torch
    from stm_amd import device_api as dev
    p = _params()
    H, W = SEQ["H"], SEQ["W"]
    f0, f1 = _sequence(3)[:2]
    z = np.zeros((H, W), np.float32)
    lib = dev.lib()
    nan = float("nan")
    cases = [("mixed_1", 3 | T, (f0, z, None), (ALPHA, THRESH_COLOR, THRESH_DISP), b"history"),
             ("mixed_2", 3 | T, (None, z, z), (ALPHA, THRESH_COLOR, THRESH_DISP), b"history"),
             ("mixed_3", 2 | T, (f0, None, None), (ALPHA, THRESH_COLOR, THRESH_DISP), b"history"),
             ("low_byte_1", 1 | T, (f0, z, z), (ALPHA, THRESH_COLOR, THRESH_DISP), b"0x2000"),
             ("low_byte_1_null", 1 | T, None, (ALPHA, THRESH_COLOR, THRESH_DISP), b"0x2000"),
             ("alpha", 3 | T, (f0, z, z), (1.5, THRESH_COLOR, THRESH_DISP), b"alpha"),
             ("alpha_nan_null", 3 | T, None, (nan, THRESH_COLOR, THRESH_DISP), b"alpha"),
             ("thresh_color", 3 | T, (f0, z, z), (ALPHA, 766, THRESH_DISP), b"thresh_color"),
             ("thresh_disp", 3 | T, (f0, z, z), (ALPHA, THRESH_COLOR, -1.0), b"thresh_disp"),
             ("thresh_disp_nan", 3 | T, (f0, z, z), (ALPHA, THRESH_COLOR, nan), b"thresh_disp"),
             ("with_0x300", 3 | T | SUBPIXEL | HSLO, (f0, z, z), (ALPHA, THRESH_COLOR, THRESH_DISP), b"0x200"),
             ("with_0x1000", 3 | T | 0x1000, (f0, z, z), (ALPHA, THRESH_COLOR, THRESH_DISP), b"0x1000")]
    lib.stm_set_error_mode(1)
    try:
        for name, stages, hist, params, word in cases:
            _arm(lib)
            dl, dr, out = _run_t(f1, p, stages, hist, params, fill=7)
            err = lib.stm_last_error()
            assert err and b"d_adcensus_stm_t" in err and word in err, (name, err)
            assert np.all(dl == 7) and np.all(dr == 7) and np.all(out == 7), name
        # num_cols_sbs < 2 * num_cols, and a history map that aliases an output: through the C ABI
        d_sbs, d_prev = torch.from_numpy(np.array(f1)).cuda(), torch.from_numpy(np.array(f0)).cuda()
        dl = torch.full((H, W), 7.0, dtype=torch.float32, device="cuda")
        dr, ql, qr = torch.full_like(dl, 7.0), torch.full_like(dl, 7.0), torch.full_like(dl, 7.0)
        out = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda")
        dev._use_current_stream()

        def call(wsbs, a, b, c, d, stages=3 | T):
            _arm(lib)
            lib.stm_d_adcensus_stm_t(dev._p(d_sbs), dev._p(a), dev._p(b), dev._p(out), H, wsbs, W, H, W, 3, p.num_views, p.angle, p.num_disp,
                                     p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, stages,
                                     dev._p(d_prev), dev._p(c), dev._p(d), ALPHA, THRESH_COLOR, THRESH_DISP)
            torch.cuda.synchronize()
            return lib.stm_last_error()

        err = call(2 * W - 1, dl, dr, ql, qr)
        assert err and b"num_cols_sbs" in err and b"d_adcensus_stm_t" in err, err
        for a, b, c, d in ((dl, dr, dl, qr), (dl, dr, ql, dr), (dl, dr, dr, ql), (dl, dr, qr, dl)):
            err = call(2 * W, a, b, c, d)
            assert err and b"alias" in err and b"d_adcensus_stm_t" in err, err
        # the bit handed to the calls that have no history arguments
        for stages in (3 | T, 2 | T):
            _arm(lib)
            g = _run(f1, p, stages, fill=7)
            err = lib.stm_last_error()
            assert err and b"0x2000" in err and b"d_adcensus_stm:" in err, err
            assert all(np.all(x == 7) for x in g)
        _arm(lib)
        dev.d_adcensus_stm_2s(d_sbs, dl, dr, out, p, H // 2, W // 2, 0.5, stages=3 | T)
        torch.cuda.synchronize()
        err = lib.stm_last_error()
        assert err and b"d_adcensus_stm_2s" in err and b"stages" in err, err
        from stm_amd import host_api as api
        _arm(lib)
        got = api.adcensus_stm_2s(np.array(f1), W, H, W, H // 2, W // 2, 0.5, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff,
                                  p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, stages=3 | T)
        err = lib.stm_last_error()
        assert err and b"adcensus_stm_2s" in err and not any(a.any() for a in got), err
    finally:
        lib.stm_set_error_mode(0)
    torch.cuda.synchronize()
    for t in (dl, dr, ql, qr):
        assert bool((t == 7).all())
    assert bool((out == 7).all())


# ----------------------------------------------------------------------------- 3. the frame stream
def _stream(frames, p, stages, temporal=None, check_setters=False):
    """the frames through a video.FrameStream, two in flight; returns the collected (index, disp_l, disp_r, interlaced)"""
    from stm_amd import device_api as dev, video
    lib = dev.lib()
    fs = video.FrameStream(SEQ["H"], SEQ["W"], p, stages=stages)
    try:
        if temporal is not None:
            fs.set_temporal(*temporal)
        got, pending = [], 0
        for f in frames:
            if pending == 2:
                got.append(fs.collect())
                pending -= 1
            assert fs.submit(f) >= 0
            pending += 1
            if check_setters and len(got) == 0 and pending == 1:
                lib.stm_set_error_mode(1)
                try:
                    _arm(lib)
                    assert lib.stm_stream_set_temporal(fs._h, 0.5, 24, 1.5) == -1
                    assert b"first submit" in lib.stm_last_error()
                    _arm(lib)
                    assert lib.stm_stream_set_stages(fs._h, 3 | T) == -1
                    assert b"first submit" in lib.stm_last_error()
                    with pytest.raises(ValueError):
                        fs.set_temporal(0.5, 24, 1.5)
                finally:
                    lib.stm_set_error_mode(0)
        while pending:
            got.append(fs.collect())
            pending -= 1
    finally:
        fs.close()
    assert [g[0] for g in got] == list(range(len(frames)))
    return got


def stream_check(n=7, temporal=None):
    """n frames through a stream with 3 | 0x2000: every collected frame equals the recursion of stm_d_adcensus_stm_t calls on the
    same inputs (the eager, captured and replayed frames of both slots).  Also run in child processes, see below."""
    p = _params()
    frames = mixed_sequence(n)
    got = _stream(frames, p, 3 | T, temporal)
    want = _recursion_t(frames, p, 3 | T, temporal or (ALPHA, THRESH_COLOR, THRESH_DISP))
    for k in range(n):
        for a, b in zip(got[k][1:], want[k]):
            assert np.array_equal(a, b), k
    return frames, got


def test_stream_with_temporal(gpu_ready):
    from stm_amd import device_api as dev, video
    p = _params()
    frames, got = stream_check(7)
    base = _stream(frames, p, 3, check_setters=True)
    assert np.array_equal(got[0][1], base[0][1]) and np.array_equal(got[0][3], base[0][3])  # the first frame has no history
    assert any(not np.array_equal(got[k][1], base[k][1]) for k in range(1, 7))
    # the parameters reach the frames; bad ones and unknown bits are refused
    stream_check(5, (0.25, 30, 0.75))
    lib = dev.lib()
    fs = video.FrameStream(SEQ["H"], SEQ["W"], p)
    lib.stm_set_error_mode(1)
    try:
        _arm(lib)
        for bad, word in (((1.5, 24, 1.5), b"alpha"), ((0.5, 766, 1.5), b"thresh_color"), ((0.5, 24, float("nan")), b"thresh_disp")):
            _arm(lib)
            assert lib.stm_stream_set_temporal(fs._h, *bad) == -1
            assert word in lib.stm_last_error()
        assert lib.stm_stream_set_temporal(fs._h, 1.0, 765, float("inf")) == 0
        assert lib.stm_stream_set_stages(fs._h, 3 | T | HSLO) == -1 and lib.stm_stream_set_stages(fs._h, 2 | T) == -1
        assert lib.stm_stream_set_stages(fs._h, 3 | T | 0x4000) == -1
        _arm(lib)
        assert lib.stm_stream_set_stages(fs._h, 3 | T | SUBPIXEL | INTERP | LINEAR_WARP) == 0
    finally:
        lib.stm_set_error_mode(0)
        fs.close()


@pytest.mark.parametrize("env", [{"STM_STREAM_OVERLAP": "0"}, {"STM_STREAM_GRAPH": "0"}], ids=["overlap_0", "graph_0"])
def test_stream_with_temporal_in_a_child_process(gpu_ready, env):
    """one compute stream and workspace for both slots, and no captured graphs: both switches are read when the stream is
    created, so a child process per mode (as test_gpu_parity's overlap test starts its children)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_temporal as t\n"
            "t.stream_check(7)\n"
            "print('ok')\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ----------------------------------------------------------------------------- 4. the default path
def test_default_path_untouched(gpu_ready, orc):
    """stm_d_adcensus_stm and a stream without the bit give the oracle's adcensus_stm before the bit is used, between two uses
    of it and after them"""
    p = _params()
    H, W = SEQ["H"], SEQ["W"]
    frames = _sequence(3)
    oracle = [orc.adcensus_stm(np.array(f), H, W, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd,
                               p.usd, p.lsd, p.thresh_s, p.thresh_h) for f in frames]
    want = [(o["disp_l"], o["disp_r"], o["interlaced"]) for o in oracle]

    def default_path():
        one = [_run(f, p, 3) for f in frames]
        stream = _stream(frames, p, 3)
        for k in range(3):
            assert all(np.array_equal(a, b) for a, b in zip(one[k], want[k])), k
            assert all(np.array_equal(a, b) for a, b in zip(stream[k][1:], want[k])), k

    default_path()
    with_bit = _recursion_t(frames, p, 3 | T)
    assert not np.array_equal(with_bit[2][0], want[2][0])
    default_path()
    _stream(frames, p, 3 | T)
    default_path()


# ----------------------------------------------------------------------------- 5. the video driver
def test_video_cli_with_temporal(gpu_ready, tmp_path):
    """tools/stm_video.py --temporal with its three optional parameters: the frames it writes are the recursion's"""
    from stm_amd import bmp_io, device_api as dev
    H, W, s = SEQ["H"], SEQ["W"], SEQ
    frames = _sequence(3)
    for k, f in enumerate(frames):
        bmp_io.write_bmp(str(tmp_path / ("f%03d.bmp" % k)), np.array(f))
    out = tmp_path / "o"
    args = [sys.executable, os.path.join(ROOT, "tools", "stm_video.py"), str(tmp_path), "8", "18.43", str(W), str(H), str(s["D"]), str(s["zd"]),
            "10", "30", "6", "20", str(s["usd"]), str(s["lsd"]), "20", "0.4", str(out), "--temporal", "--temporal-alpha", "0.25",
            "--temporal-color", "30", "--temporal-disp", "0.75"]
    subprocess.check_call(args)
    p = dev.FrameParams(num_disp=s["D"], zero_disp=s["zd"], usd=s["usd"], lsd=s["lsd"], angle=18.0)  # the tool truncates the slant
    want = _recursion_t(frames, p, 3 | T, (0.25, 30, 0.75))
    plain = _run(frames[2], p, 3)
    for k in range(3):
        assert np.array_equal(bmp_io.read_bmp(str(out / ("interlaced_%05d.bmp" % k))), want[k][2]), k
    assert not np.array_equal(want[2][0], plain[0])
    # a parameter without --temporal is refused before anything runs
    assert subprocess.call(args[:-7] + ["--temporal-alpha", "0.25"], stdout=subprocess.DEVNULL) != 0
