"""NV12 input on the GPU: the conversion + split as a stage (stm_demux_nv12 / stm_d_demux_nv12), the device-resident frame
(stm_d_adcensus_stm_nv12) and the frame stream in NV12 mode (stm_stream_set_input), every comparison bit for bit: the stage against
the numpy statement of the definition (test_nv12_ref.nv12_to_bgr_ref), the frame and the stream against the existing BGR calls
applied to the frame that statement gives."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_nv12_ref import nv12_frame, nv12_halves, nv12_to_bgr_ref, random_planes
from test_temporal_ref import ALPHA, SEQ, THRESH_COLOR, THRESH_DISP, mixed_sequence

pytestmark = pytest.mark.gpu

T, SUBPIXEL, INTERP, LINEAR_WARP, HSLO = 0x2000, 0x200, 0x400, 0x800, 0x100
FILL = 0x5A


def _arm(lib):
    """plant a known message (error mode 1): a later check sees the call's own message or this one, never an earlier test's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


def _no_new_error(lib):
    return b"d_filter_median" in lib.stm_last_error()


def _params():
    from stm_amd import device_api as dev
    s = SEQ
    return dev.FrameParams(num_disp=s["D"], zero_disp=s["zd"], usd=s["usd"], lsd=s["lsd"])


_SEQ = {}


def _sequence(n, matrix=0):
    """n NV12 frames of the temporal tests' sequence (40 x 72 per view) with the BGR side-by-side frames the definition gives;
    computed once, read only"""
    from stm_amd import synth
    if (n, matrix) not in _SEQ:
        nv = [synth.bgr_to_nv12(f, matrix) for f in mixed_sequence(n)]
        bgr = [nv12_to_bgr_ref(y, uv, matrix) for y, uv in nv]
        for a in [x for pair in nv for x in pair] + bgr:
            a.setflags(write=False)
        _SEQ[(n, matrix)] = (nv, bgr)
    return _SEQ[(n, matrix)]


# ----------------------------------------------------------------------------- 1. the stage
# (H, W, Wsbs - 2W, pitch_y - Wsbs, pitch_uv - Wsbs, odd base offsets)
STAGE_CASES = [(2, 2, 0, 0, 0, False), (2, 6, 0, 0, 0, False), (16, 64, 0, 0, 0, False), (18, 66, 0, 0, 0, False), (20, 200, 0, 0, 0, False),
               (34, 130, 4, 6, 2, True)]
STAGE_IDS = ["%dx%d" % c[:2] for c in STAGE_CASES]


def _host_view(a, pitch, odd):
    """the rows of `a` at pitch `pitch` inside a larger host buffer of other bytes, the first at an odd address if asked"""
    H, n = a.shape
    buf = np.full(H * pitch + 64, 0xC3, np.uint8)
    off = (1 - buf.ctypes.data) % 2 if odd else 0
    off += 2 if odd and off == 0 else 0
    v = np.lib.stride_tricks.as_strided(buf[off:], shape=(H, n), strides=(pitch, 1))
    v[...] = a
    assert not odd or v.ctypes.data % 2 == 1
    return v, buf, off


@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("case", STAGE_CASES, ids=STAGE_IDS)
def test_demux_nv12_both_flavours(gpu_ready, stm, case, elem_sz):
    import torch
    from test_gpu_caller_buffers import Arena, P, read
    from stm_amd import host_api as api
    H, W, spare, py_extra, puv_extra, odd = case
    Wsbs = 2 * W + spare
    pitch_y, pitch_uv = Wsbs + py_extra, Wsbs + puv_extra
    assert not odd or (pitch_y == 2 * W + 10 and pitch_uv == 2 * W + 6)
    y, uv = random_planes(H * 7 + W, H, Wsbs, pitch_y, pitch_uv)
    for plane in (y, uv[:, 0::2], uv[:, 1::2]):
        assert plane.min() == 0 and plane.max() == 255
    lib = stm.lib()
    lib.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for matrix in range(4):
        want = nv12_halves(y, uv, W, matrix, elem_sz)
        # host flavour: pitched views, bytes past a pixel's third come back 0
        hy, ybuf, yoff = _host_view(y, pitch_y, odd)
        huv, uvbuf, uvoff = _host_view(uv, pitch_uv, odd)
        keep = ybuf.copy(), uvbuf.copy()
        got = api.demux_nv12(hy, huv, W, elem_sz, matrix, num_cols_sbs=Wsbs)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), ("host", matrix)
        assert np.array_equal(ybuf, keep[0]) and np.array_equal(uvbuf, keep[1])
        # device flavour: every buffer inside one arena (guard bands), planes pitched, bases odd where the case says so
        arena = Arena(True, nbytes=1 << 20)
        d_y = arena.put(np.ascontiguousarray(ybuf[yoff:yoff + H * pitch_y]), 1 if odd else 0)
        d_uv = arena.put(np.ascontiguousarray(uvbuf[uvoff:uvoff + (H // 2) * pitch_uv]), 3 if odd else 0)
        d_l = arena.put(np.full((H, W, elem_sz), FILL, np.uint8), 5 if odd else 0)
        d_r = arena.put(np.full((H, W, elem_sz), FILL, np.uint8), 7 if odd else 4)
        lib.stm_d_demux_nv12(P(d_l), P(d_r), P(d_y), pitch_y, P(d_uv), pitch_uv, H, Wsbs, W, elem_sz, matrix)
        assert arena.intact(), ("guard bands", matrix)
        for d, w in ((d_l, want[0]), (d_r, want[1])):
            g = read(d, np.uint8, (H, W, elem_sz))
            assert np.array_equal(g[:, :, :3], w[:, :, :3]), ("device", matrix)
            assert (g[:, :, 3:] == FILL).all()  # left to the caller
        assert np.array_equal(read(d_y, np.uint8, (H * pitch_y,)), ybuf[yoff:yoff + H * pitch_y])
        assert np.array_equal(read(d_uv, np.uint8, ((H // 2) * pitch_uv,)), uvbuf[uvoff:uvoff + (H // 2) * pitch_uv])


def test_demux_nv12_seam(gpu_ready, stm):
    """left half white, right half black: no column of either view next to the seam differs from the view's interior"""
    import torch
    from stm_amd import device_api as dev, host_api as api
    H, W = 18, 66
    y = np.concatenate([np.full((H, W), 235, np.uint8), np.full((H, W), 16, np.uint8)], axis=1)
    uv = np.full((H // 2, 2 * W), 128, np.uint8)
    l, r = api.demux_nv12(y, uv, W)
    assert (l == 255).all() and (r == 0).all()
    dl = torch.full((H, W, 3), FILL, dtype=torch.uint8, device="cuda")
    dr = torch.full_like(dl, FILL)
    dev.d_demux_nv12(dl, dr, torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())
    torch.cuda.synchronize()
    assert bool((dl == 255).all()) and bool((dr == 0).all())


# ----------------------------------------------------------------------------- 2. / 3. the frame
def _nv12_call(y, uv, p, stages, matrix=0, hist=None, images=True, fill=0, params=(ALPHA, THRESH_COLOR, THRESH_DISP), W=None):
    """stm_d_adcensus_stm_nv12 on buffers pre-filled with `fill`; hist = (prev img_l, prev img_r, prev disp_l, prev disp_r) or None.
    Returns (disp_l, disp_r, interlaced, img_l, img_r); the last two None without `images`."""
    import torch
    from stm_amd import device_api as dev
    H = y.shape[0]
    W = W or y.shape[1] // 2
    d_y, d_uv = torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(np.array(uv)).cuda()
    dl = torch.full((H, W), float(fill), dtype=torch.float32, device="cuda")
    dr = torch.full_like(dl, float(fill))
    out = torch.full((H, W, 3), fill, dtype=torch.uint8, device="cuda")
    il = torch.full((H, W, 3), fill, dtype=torch.uint8, device="cuda") if images else None
    ir = torch.full((H, W, 3), fill, dtype=torch.uint8, device="cuda") if images else None
    h = [None] * 4 if hist is None else [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in hist]
    dev.d_adcensus_stm_nv12(d_y, d_uv, dl, dr, out, p, stages, matrix, il, ir, h[0], h[1], h[2], h[3], *params)
    torch.cuda.synchronize()
    assert np.array_equal(d_y.cpu().numpy(), y) and np.array_equal(d_uv.cpu().numpy(), uv)  # the planes are read only
    if hist is not None:
        for a, t in zip(hist, h):
            assert a is None or np.array_equal(a, t.cpu().numpy())
    return (dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy(), None if il is None else il.cpu().numpy(),
            None if ir is None else ir.cpu().numpy())


def _bgr_call(sbs, p, stages, hist=None, fill=0):
    """stm_d_adcensus_stm (without 0x2000) / stm_d_adcensus_stm_t (with it) on the BGR frame; hist = (prev sbs, prev dl, prev dr)"""
    import torch
    from stm_amd import device_api as dev
    H, W = sbs.shape[0], sbs.shape[1] // 2
    d_sbs = torch.from_numpy(np.array(sbs)).cuda()
    dl = torch.full((H, W), float(fill), dtype=torch.float32, device="cuda")
    dr = torch.full_like(dl, float(fill))
    out = torch.full((H, W, 3), fill, dtype=torch.uint8, device="cuda")
    if stages & T:
        h = [None] * 3 if hist is None else [torch.from_numpy(np.array(a)).cuda() for a in hist]
        dev.d_adcensus_stm_t(d_sbs, dl, dr, out, p, stages, h[0], h[1], h[2], ALPHA, THRESH_COLOR, THRESH_DISP)
    else:
        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("shape", [(18, 66), (40, 72)], ids=["18x66", "40x72"])
def test_fused_against_plain(gpu_ready, stm, shape):
    """the frame with the conversion inside stm_k_front_nv12 (variant 0) and with stm_k_demux_nv12 followed by the unfused kernels
    (variant 600): equal maps, split images and interlaced frame; and the same without output images"""
    H, W = shape
    p = _params()
    y, uv = random_planes(H + W, H, 2 * W) if shape != (40, 72) else _sequence(5)[0][1]
    lib = stm.lib()
    a = _nv12_call(y, uv, p, 3)
    try:
        lib.stm_set_agg_variant(600)
        b = _nv12_call(y, uv, p, 3)
    finally:
        lib.stm_set_agg_variant(0)
    for k in range(5):
        assert np.array_equal(a[k], b[k]), k
    want = nv12_halves(y, uv, W)
    assert np.array_equal(a[3], want[0]) and np.array_equal(a[4], want[1])
    c = _nv12_call(y, uv, p, 3, images=False)
    for k in range(3):
        assert np.array_equal(a[k], c[k]), k


@pytest.mark.parametrize("elem_sz", [3, 4])
def test_fused_against_plain_pitched_planes(gpu_ready, stm, elem_sz):
    """34 x 130 with Wsbs = 2W + 4, pitch_y = 2W + 10, pitch_uv = 2W + 6, both planes and both output images at odd addresses inside
    one arena: the terms of stm_k_front_nv12's fetch that coincide when Wsbs == 2W == pitch.  Split images against the definition,
    maps and interlaced frame against variant 600 (stm_k_demux_nv12 + the unfused kernels); the guard bands and planes stay"""
    import torch
    from test_gpu_caller_buffers import Arena, P, read
    H, W = 34, 130
    Wsbs, pitch_y, pitch_uv = 2 * W + 4, 2 * W + 10, 2 * W + 6
    y, uv = random_planes(991 + elem_sz, H, Wsbs, pitch_y, pitch_uv)
    ybuf = np.full(H * pitch_y, 0xC3, np.uint8)
    uvbuf = np.full((H // 2) * pitch_uv, 0xC3, np.uint8)
    ybuf.reshape(H, pitch_y)[:, :Wsbs] = y
    uvbuf.reshape(H // 2, pitch_uv)[:, :uv.shape[1]] = uv
    want = nv12_halves(y, uv, W, 1, elem_sz)
    p = _params()
    lib = stm.lib()
    lib.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    got = {}
    try:
        for variant in (0, 600):
            lib.stm_set_agg_variant(variant)
            arena = Arena(True, nbytes=1 << 20)
            d_y, d_uv = arena.put(ybuf, 1), arena.put(uvbuf, 3)
            d_il, d_ir = arena.put(np.full((H, W, elem_sz), FILL, np.uint8), 5), arena.put(np.full((H, W, elem_sz), FILL, np.uint8), 7)
            d_dl, d_dr = arena.put(np.zeros((H, W), np.float32), 4), arena.put(np.zeros((H, W), np.float32), 12)
            d_out = arena.put(np.full((H, W, elem_sz), FILL, np.uint8), 9)
            lib.stm_d_adcensus_stm_nv12(P(d_y), pitch_y, P(d_uv), pitch_uv, 1, P(d_dl), P(d_dr), P(d_out), H, Wsbs, W, H, W, elem_sz,
                                        p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                                        p.thresh_s, p.thresh_h, 3, None, None, None, None, ALPHA, THRESH_COLOR, THRESH_DISP, P(d_il), P(d_ir))
            assert arena.intact(), variant
            assert np.array_equal(read(d_y, np.uint8, ybuf.shape), ybuf) and np.array_equal(read(d_uv, np.uint8, uvbuf.shape), uvbuf)
            for d, w in ((d_il, want[0]), (d_ir, want[1])):
                g = read(d, np.uint8, (H, W, elem_sz))
                assert np.array_equal(g[:, :, :3], w[:, :, :3]), variant
                assert (g[:, :, 3:] == FILL).all()  # left to the caller
            got[variant] = (read(d_dl, np.float32, (H, W)), read(d_dr, np.float32, (H, W)), read(d_out, np.uint8, (H, W, elem_sz))[:, :, :3])
    finally:
        lib.stm_set_agg_variant(0)
    for a, b in zip(got[0], got[600]):
        assert np.array_equal(a, b)
    assert got[0][0].any() and got[0][2].any()


STAGE_WORDS = [1, 2, 3, 3 | HSLO, 3 | SUBPIXEL | INTERP | LINEAR_WARP]


@pytest.mark.parametrize("matrix", [0, 3])
@pytest.mark.parametrize("stages", STAGE_WORDS, ids=["0x%x" % s for s in STAGE_WORDS])
def test_frame_equals_the_bgr_frame(gpu_ready, stages, matrix):
    """40 x 72, D = 8: stm_d_adcensus_stm_nv12 equals stm_d_adcensus_stm on the BGR frame nv12_to_bgr_ref builds"""
    p = _params()
    nv, bgr = _sequence(5, matrix)
    got = _nv12_call(*nv[1], p, stages, matrix)
    want = _bgr_call(bgr[1], p, stages)
    for k in range(3):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got[3], bgr[1][:, :SEQ["W"]]) and np.array_equal(got[4], bgr[1][:, SEQ["W"]:])
    assert got[0].any() and (got[2].any() == ((stages & 0xff) == 3))


def test_frame_with_history(gpu_ready):
    """3 | 0x2000, three frames, each with the previous frame's split images and maps as its history: equal to the recursion of
    stm_d_adcensus_stm_t on the BGR frames; a first frame with all history pointers null equals the call without the bit"""
    p = _params()
    nv, bgr = _sequence(5)
    got, want = [], []
    for k in range(3):
        got.append(_nv12_call(*nv[k], p, 3 | T, hist=None if k == 0 else (got[-1][3], got[-1][4], got[-1][0], got[-1][1])))
        want.append(_bgr_call(bgr[k], p, 3 | T, None if k == 0 else (bgr[k - 1], want[-1][0], want[-1][1])))
        for j in range(3):
            assert np.array_equal(got[k][j], want[k][j]), (k, j)
    plain = _nv12_call(*nv[0], p, 3)
    for j in range(5):
        assert np.array_equal(got[0][j], plain[j]), j
    assert not np.array_equal(got[2][0], _nv12_call(*nv[2], p, 3)[0])  # the step did something
    # without the bit the history is ignored
    z = np.zeros((SEQ["H"], SEQ["W"]), np.float32)
    a = _nv12_call(*nv[1], p, 3, hist=(got[0][3], got[0][4], z, z))
    assert all(np.array_equal(x, q) for x, q in zip(a, _nv12_call(*nv[1], p, 3)))


# ----------------------------------------------------------------------------- 4. the stream
def _stream(frames, p, stages, input_format, inplace=False, matrix=0):
    from stm_amd import video
    fs = video.FrameStream(SEQ["H"], SEQ["W"], p, stages=stages, input_format=input_format, matrix=matrix)
    try:
        got, pending = [], 0
        for f in frames:
            if pending == 2:
                got.append(fs.collect())
                pending -= 1
            if inplace:
                buf = fs.input_buffer()
                assert buf is not None and buf.shape == f.shape
                buf[...] = f
                assert fs.submit_inplace() >= 0
            else:
                assert fs.submit(f) >= 0
            pending += 1
        while pending:
            got.append(fs.collect())
            pending -= 1
    finally:
        fs.close()
    assert [g[0] for g in got] == list(range(len(frames)))
    return got


@pytest.mark.parametrize("inplace", [False, True], ids=["submit", "input_buffer"])
@pytest.mark.parametrize("stages", [3, 3 | SUBPIXEL | LINEAR_WARP | T], ids=["0x3", "0x2a03"])
def test_stream_in_nv12_mode(gpu_ready, stages, inplace):
    """five NV12 frames, two in flight: every collected frame equals the recursion of the per-frame calls (the fifth frame
    replays its slot's captured graph); a BGR-mode stream created afterwards still equals stm_d_adcensus_stm"""
    p = _params()
    nv, bgr = _sequence(5)
    got = _stream([nv12_frame(y, uv) for y, uv in nv], p, stages, "nv12", inplace)
    want = []
    for k in range(5):
        hist = None if k == 0 or not stages & T else (want[-1][3], want[-1][4], want[-1][0], want[-1][1])
        want.append(_nv12_call(*nv[k], p, stages, hist=hist))
        for j in range(3):
            assert np.array_equal(got[k][1 + j], want[k][j]), (k, j)
    after = _stream(bgr[:3], p, 3, "bgr", inplace)
    for k in range(3):
        for a, b in zip(after[k][1:], _bgr_call(bgr[k], p, 3)):
            assert np.array_equal(a, b), k


# ----------------------------------------------------------------------------- 5. errors
def test_stage_errors(gpu_ready, stm):
    import torch
    lib = stm.lib()
    u8p = C.POINTER(C.c_uint8)
    H, W = 4, 6
    y, uv = random_planes(1, H, 2 * W)
    y, uv = np.ascontiguousarray(y), np.ascontiguousarray(uv)
    hl, hr = np.full((H, W, 3), 7, np.uint8), np.full((H, W, 3), 7, np.uint8)
    d_y, d_uv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    dl = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda")
    dr = torch.full_like(dl, 7)
    # (pitch_y, pitch_uv, num_rows, num_cols_sbs, num_cols_out, elem_sz, matrix), the word the message must carry
    bad = [((12, 12, 3, 12, 6, 3, 0), b"num_rows"), ((12, 12, 4, 12, 5, 3, 0), b"num_cols_out"), ((12, 12, 4, 11, 6, 3, 0), b"num_cols_sbs"),
           ((11, 12, 4, 12, 6, 3, 0), b"pitch_y"), ((12, 11, 4, 12, 6, 3, 0), b"pitch_uv"), ((13, 13, 4, 13, 6, 3, 0), b"pitch_uv"),
           ((12, 12, 4, 12, 6, 3, 4), b"matrix"), ((12, 12, 4, 12, 6, 3, -1), b"matrix"), ((12, 12, 4, 12, 6, 2, 0), b"elem_sz"),
           ((12, 12, 0, 12, 6, 3, 0), b"num_rows"), ((12, 12, 4, 12, 0, 3, 0), b"num_cols_out")]
    lib.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    lib.stm_set_error_mode(1)
    try:
        for (py, puv, rows, wsbs, w, e, m), word in bad:
            _arm(lib)
            lib.stm_demux_nv12(hl.ctypes.data_as(u8p), hr.ctypes.data_as(u8p), y.ctypes.data_as(u8p), py, uv.ctypes.data_as(u8p), puv, rows, wsbs, w, e, m)
            err = lib.stm_last_error()
            assert err and word in err and b"demux_nv12" in err and b"d_demux_nv12" not in err, (word, err)
            _arm(lib)
            lib.stm_d_demux_nv12(dl.data_ptr(), dr.data_ptr(), d_y.data_ptr(), py, d_uv.data_ptr(), puv, rows, wsbs, w, e, m)
            err = lib.stm_last_error()
            assert err and word in err and b"d_demux_nv12" in err, (word, err)
        # the limits themselves are legal: the last matrix, and an odd num_cols_sbs with the pitch the rule gives
        _arm(lib)
        lib.stm_d_demux_nv12(dl.data_ptr(), dr.data_ptr(), d_y.data_ptr(), 12, d_uv.data_ptr(), 12, 4, 12, 6, 3, 3)
        torch.cuda.synchronize()
        assert _no_new_error(lib)
        dl.fill_(7)
        dr.fill_(7)
        lib.stm_d_demux_nv12(dl.data_ptr(), dr.data_ptr(), d_y.data_ptr(), 12, d_uv.data_ptr(), 12, 4, 11, 4, 3, 0)
        torch.cuda.synchronize()
        flat = dl.flatten()  # 4 x 4 pixels of the narrower view, dense from the buffer's start; the rest is untouched
        assert _no_new_error(lib) and not bool((flat[:48] == 7).all()) and bool((flat[48:] == 7).all())
        dl.fill_(7)
        dr.fill_(7)
    finally:
        lib.stm_set_error_mode(0)
    torch.cuda.synchronize()
    assert (hl == 7).all() and (hr == 7).all() and bool((dl == 7).all()) and bool((dr == 7).all())


def test_frame_errors(gpu_ready):
    """every rule is reported with the call's name and the argument's before anything is launched: the buffers keep their fill"""
    import torch
    from stm_amd import device_api as dev
    lib = dev.lib()
    p = _params()
    H, W = SEQ["H"], SEQ["W"]
    nv, _ = _sequence(5)
    y, uv = nv[1]
    d_y, d_uv = torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(np.array(uv)).cuda()

    def f32():
        return torch.full((H, W), 7.0, dtype=torch.float32, device="cuda")

    def u8():
        return torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda")
    dl, dr, ql, qr = f32(), f32(), f32(), f32()
    out, il, ir, pil, pir = u8(), u8(), u8(), u8(), u8()
    dev._use_current_stream()

    def call(stages=3, rows=H, wsbs=2 * W, w=W, py=2 * W, puv=2 * W, m=0, imgs=(il, ir), hist=(None, None, None, None), alpha=ALPHA, outs=(dl, dr)):
        _arm(lib)
        ptr = lambda t: None if t is None else dev._p(t)  # noqa: E731
        lib.stm_d_adcensus_stm_nv12(dev._p(d_y), py, dev._p(d_uv), puv, m, dev._p(outs[0]), dev._p(outs[1]), dev._p(out), rows, wsbs, w, H, W, 3,
                                    p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                                    p.thresh_s, p.thresh_h, stages, ptr(hist[0]), ptr(hist[1]), ptr(hist[2]), ptr(hist[3]), alpha,
                                    THRESH_COLOR, THRESH_DISP, ptr(imgs[0]), ptr(imgs[1]))
        torch.cuda.synchronize()
        return lib.stm_last_error()

    full = (pil, pir, ql, qr)
    cases = [("odd rows", dict(rows=H - 1), b"num_rows"), ("odd cols", dict(w=W - 1), b"num_cols"),
             ("narrow frame", dict(wsbs=2 * W - 2), b"num_cols_sbs"), ("pitch_y", dict(py=2 * W - 1), b"pitch_y"),
             ("pitch_uv", dict(puv=2 * W - 1), b"pitch_uv"), ("matrix", dict(m=4), b"matrix"), ("matrix", dict(m=-1), b"matrix"),
             ("one image", dict(imgs=(il, None)), b"d_img_r"), ("other image", dict(imgs=(None, ir)), b"d_img_l"),
             ("0x2000 without images", dict(stages=3 | T, imgs=(None, None)), b"d_img_l"),
             ("0x2000 without images, history", dict(stages=3 | T, imgs=(None, None), hist=full), b"d_img_l"),
             ("mixed history 1", dict(stages=3 | T, hist=(pil, pir, ql, None)), b"history"),
             ("mixed history 2", dict(stages=3 | T, hist=(None, pir, ql, qr)), b"history"),
             ("mixed history 3", dict(stages=2 | T, hist=(pil, None, None, None)), b"history"),
             ("history image is an output", dict(stages=3 | T, hist=(il, pir, ql, qr)), b"alias"),
             ("history image is the other output", dict(stages=3 | T, hist=(pil, il, ql, qr)), b"alias"),
             ("history map is an output", dict(stages=3 | T, hist=(pil, pir, dr, qr)), b"alias"),
             ("history map is the other output", dict(stages=3 | T, hist=(pil, pir, ql, dl)), b"alias"),
             ("low byte 1", dict(stages=1 | T, hist=full), b"0x2000"), ("alpha", dict(stages=3 | T, hist=full, alpha=1.5), b"alpha"),
             ("0x300", dict(stages=3 | SUBPIXEL | HSLO), b"0x200"), ("0x1000", dict(stages=3 | 0x1000), b"0x1000"),
             ("0x400 with 1", dict(stages=1 | INTERP), b"0x400"), ("0x800 with 2", dict(stages=2 | LINEAR_WARP), b"0x800")]
    lib.stm_set_error_mode(1)
    try:
        for name, kw, word in cases:
            err = call(**kw)
            assert err and b"d_adcensus_stm_nv12" in err and word in err, (name, err)
            for t in (dl, dr, ql, qr, out, il, ir, pil, pir):
                assert bool((t == 7).all()), name
        # a legal call in between launches and reports nothing
        err = call(stages=3 | T, hist=full)
        assert _no_new_error(lib), err
    finally:
        lib.stm_set_error_mode(0)


def test_stream_input_errors(gpu_ready):
    from stm_amd import device_api as dev, video
    lib = dev.lib()
    p = _params()
    nv, _ = _sequence(5)
    lib.stm_set_error_mode(1)
    try:
        fs = video.FrameStream(SEQ["H"], SEQ["W"], p)
        try:
            for fmt, m, word in ((2, 0, b"format"), (-1, 0, b"format"), (1, 4, b"matrix"), (1, -1, b"matrix")):
                _arm(lib)
                assert lib.stm_stream_set_input(fs._h, fmt, m) == -1
                err = lib.stm_last_error()
                assert b"stream_set_input" in err and word in err, err
            with pytest.raises(ValueError):
                fs.set_input("i420")
            _arm(lib)
            assert lib.stm_stream_set_input(fs._h, 1, 3) == 0 and lib.stm_stream_set_input(fs._h, 0, 9) == 0  # matrix is ignored for BGR
            assert lib.stm_stream_set_stages(fs._h, 3 | 0x4000) == -1  # an input format, not a stage bit
            fs.set_input("nv12", 0)
            assert fs.submit(nv12_frame(*nv[0])) == 0
            _arm(lib)
            assert lib.stm_stream_set_input(fs._h, 0, 0) == -1
            err = lib.stm_last_error()
            assert b"stream_set_input" in err and b"first submit" in err, err
            assert fs.collect()[0] == 0
        finally:
            fs.close()
        for rows, cols, word in ((SEQ["H"] + 1, SEQ["W"], b"num_rows"), (SEQ["H"], SEQ["W"] + 1, b"num_cols")):
            fs = video.FrameStream(rows, cols, p)
            try:
                _arm(lib)
                assert lib.stm_stream_set_input(fs._h, 1, 0) == -1
                err = lib.stm_last_error()
                assert b"stream_set_input" in err and word in err, err
            finally:
                fs.close()
    finally:
        lib.stm_set_error_mode(0)


# ----------------------------------------------------------------------------- the video driver
def test_video_cli_with_nv12(gpu_ready, tmp_path):
    """tools/stm_video.py --nv12 ROWS COLS_SBS --matrix M on a raw .yuv file: the frames it writes are the per-frame calls'"""
    import os
    import sys
    from conftest import ROOT
    from stm_amd import bmp_io, device_api as dev
    H, W, s = SEQ["H"], SEQ["W"], SEQ
    nv, _ = _sequence(5, 3)
    clip = tmp_path / "clip.yuv"
    clip.write_bytes(b"".join(nv12_frame(y, uv).tobytes() for y, uv in nv[:3]))
    out = tmp_path / "o"
    args = [sys.executable, os.path.join(ROOT, "tools", "stm_video.py"), str(clip), "8", "18.43", str(W), str(H), str(s["D"]), str(s["zd"]),
            "10", "30", "6", "20", str(s["usd"]), str(s["lsd"]), "20", "0.4", str(out), "--nv12", str(H), str(2 * W), "--matrix", "3"]
    subprocess.check_call(args)
    p = dev.FrameParams(num_disp=s["D"], zero_disp=s["zd"], usd=s["usd"], lsd=s["lsd"], angle=18.0)  # the tool truncates the slant
    for k in range(3):
        want = _nv12_call(*nv[k], p, 3, 3)
        assert np.array_equal(bmp_io.read_bmp(str(out / ("interlaced_%05d.bmp" % k))), want[2]), k
    # --matrix without --nv12 is refused before anything runs
    assert subprocess.call(args[:17] + ["--matrix", "3"], stdout=subprocess.DEVNULL) != 0


# ----------------------------------------------------------------------------- 6. the ABI
def test_library_exports_the_nv12_names(stm):
    out = subprocess.check_output(["nm", "-D", "--defined-only", stm.LIB_PATH]).decode()
    have = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    for name in ("stm_demux_nv12", "stm_d_demux_nv12", "stm_d_adcensus_stm_nv12", "stm_stream_set_input"):
        assert name in have, name
