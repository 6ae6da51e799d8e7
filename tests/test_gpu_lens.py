"""Calibrated lenticular interlacing on the GPU (stm_set_lens, stm_stream_set_lens, stm_mux_multiview_lens /
stm_d_mux_multiview_lens), bit for bit against the numpy statement of the definition (test_lens_ref) on the oracle's chain.
Every test leaves the thread's geometry at mode 0."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from test_lens_ref import (LINEAR_WARP, SUBPIXEL, frame_lens_ref, mux_lens_ref, random_views, render_chain,
                           render_lens_ref)

pytestmark = pytest.mark.gpu

T = 0x2000
PANEL = (7.37, 0.86, 0.3)       # a panel's calibration: non-integer pitch
PANEL_B = (5.5, -1.25, -0.4)    # negative slope and centre
FILL = 0x5A


@contextlib.contextmanager
def thread_lens(mode, pitch=0.0, slope=0.0, centre=0.0):
    """the calling thread's geometry for the duration of the block; mode 0 again afterwards, whatever happens"""
    from stm_amd import device_api as dev
    try:
        dev.set_lens(mode, pitch, slope, centre)
        yield
    finally:
        assert dev.lib().stm_set_lens(0, 0.0, 0.0, 0.0) == 0


def _params(D, zd, usd, lsd, N=8):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd, num_views=N)


def _run(sbs, p, stages, out_rows=None, out_cols=None, fill=0):
    import torch
    from stm_amd import device_api as dev
    H, W = sbs.shape[0], sbs.shape[1] // 2
    d_sbs = torch.from_numpy(np.array(sbs)).cuda()
    dl = torch.full((H, W), float(fill), dtype=torch.float32, device="cuda")
    dr = torch.full_like(dl, float(fill))
    out = torch.full((out_rows or H, out_cols or W, 3), fill, dtype=torch.uint8, device="cuda")
    dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _run_t(sbs, p, stages, hist):
    """stm_d_adcensus_stm_t; hist = (previous sbs, previous disp_l, previous disp_r) or None"""
    import torch
    from stm_amd import device_api as dev
    H, W = sbs.shape[0], sbs.shape[1] // 2
    d_sbs = torch.from_numpy(np.array(sbs)).cuda()
    dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    h = [None, None, None] if hist is None else [torch.from_numpy(np.array(a)).cuda() for a in hist]
    dev.d_adcensus_stm_t(d_sbs, dl, dr, out, p, stages, h[0], h[1], h[2])
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _small_frame(seed_off=0):
    from stm_amd import synth
    H, W, D, zd = 40, 64, 16, 8
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + seed_off)
    return sbs, _params(D, zd, 17, 8), H, W


# ----------------------------------------------------------------------------- 1. per stage
SIZES = [((9, 37), (9, 37)), ((1, 5), (3, 7)), ((6, 1), (6, 1)), ((20, 300), (31, 257))]  # the last: more than one 256-wide block


@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("sizes", SIZES, ids=["%dx%d_to_%dx%d" % (a + b) for a, b in SIZES])
def test_mux_lens_both_flavours(gpu_ready, sizes, elem_sz):
    """modes 1 and 2, N = 2 / 5 / 8, a non-integer pitch and a negative slope: the host flavour zeroes the padding bytes, the device
    flavour leaves them alone; the views are read only"""
    import torch
    from stm_amd import device_api as dev, host_api as api
    (H, W), (Ho, Wo) = sizes
    for N in (2, 5, 8):
        views = random_views(11 * N + H, N, H, W, elem_sz)
        keep = [v.copy() for v in views]
        d_views = [torch.from_numpy(v).cuda() for v in views]
        for mode in (1, 2):
            for geom in (PANEL, PANEL_B):
                want = mux_lens_ref(views, mode, *geom, Ho, Wo)
                got = api.mux_multiview_lens(views, mode, *geom, Ho, Wo)
                assert got.shape == (Ho, Wo, elem_sz)
                assert np.array_equal(got[..., :3], want), ("host", N, mode, geom)
                assert not got[..., 3:].any()
                out = torch.full((Ho, Wo, elem_sz), FILL, dtype=torch.uint8, device="cuda")
                dev.d_mux_multiview_lens(d_views, out, mode, *geom)
                torch.cuda.synchronize()
                got_d = out.cpu().numpy()
                assert np.array_equal(got_d[..., :3], want), ("device", N, mode, geom)
                assert (got_d[..., 3:] == FILL).all()
        for a, b, t in zip(keep, views, d_views):
            assert np.array_equal(a, b) and np.array_equal(a, t.cpu().numpy())


def test_mux_lens_at_the_references_geometry(gpu_ready, orc):
    """pitch 8, slope 1, centre 1/16 with 8 views is the reference's interlacer at its default angle"""
    from stm_amd import host_api as api
    views = random_views(3, 8, 37, 53)
    assert np.array_equal(api.mux_multiview_lens(views, 1, 8.0, 1.0, 1.0 / 16.0, 50, 81), orc.mux_multiview(views, 18.43, 50, 81))


# ----------------------------------------------------------------------------- 2. the frame
STAGE_WORDS = [3, 3 | SUBPIXEL | LINEAR_WARP]


@pytest.mark.parametrize("out_size", [(40, 64), (50, 81)], ids=["40x64", "50x81"])
@pytest.mark.parametrize("stages", STAGE_WORDS, ids=["0x%x" % s for s in STAGE_WORDS])
def test_frame_against_the_oracle_chain(gpu_ready, orc, stages, out_size):
    """stm_d_adcensus_stm, 40 x 64, D = 16, under modes 1, 2 and 3: the interlaced frame is frame_lens_ref's on the oracle chain, the
    maps are the same in every mode, stm_set_agg_variant(200) (every view written, then interlaced; mode 3 stays fused) gives the
    same bytes, and after stm_set_lens(0, ...) the call gives today's output again"""
    from stm_amd import device_api as dev
    sbs, p, H, W = _small_frame()
    Ho, Wo = out_size
    extra = stages & ~0xff
    lib = dev.lib()
    before = _run(sbs, p, stages, Ho, Wo)
    try:
        outs = {}
        for mode in (1, 2, 3):
            geom = PANEL if mode != 2 else PANEL_B
            wl, wr, want = frame_lens_ref(orc, sbs, p, (mode,) + geom, extra, Ho, Wo)
            with thread_lens(mode, *geom):
                dl, dr, out = _run(sbs, p, stages, Ho, Wo)
                lib.stm_set_agg_variant(200)
                unfused = _run(sbs, p, stages, Ho, Wo)
                lib.stm_set_agg_variant(0)
            assert np.array_equal(dl, wl) and np.array_equal(dr, wr), mode
            assert np.array_equal(dl, before[0]) and np.array_equal(dr, before[1]), mode
            assert np.array_equal(out, want), mode
            for a, b in zip(unfused, (dl, dr, out)):
                assert np.array_equal(a, b), mode
            assert not np.array_equal(out, before[2]), mode
            outs[mode] = out
        assert not np.array_equal(outs[1], outs[3])
    finally:
        lib.stm_set_agg_variant(0)
        lib.stm_set_lens(0, 0.0, 0.0, 0.0)
    after = _run(sbs, p, stages, Ho, Wo)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_frame_ignores_the_angle_under_a_lens(gpu_ready, orc):
    """angle 0 has no row period (an error for the reference's interlacer); under a lens geometry it is neither used nor screened"""
    from stm_amd import device_api as dev
    sbs, p, H, W = _small_frame()
    want = frame_lens_ref(orc, sbs, p, (3,) + PANEL)[2]
    q = dev.FrameParams(num_disp=p.num_disp, zero_disp=p.zero_disp, usd=p.usd, lsd=p.lsd, angle=0.0)
    with thread_lens(3, *PANEL):
        assert np.array_equal(_run(sbs, q, 3)[2], want)


def test_nv12_frame_in_mode_3(gpu_ready, orc):
    """stm_d_adcensus_stm_nv12: the frame of the converted BGR pair"""
    import torch
    from stm_amd import device_api as dev, synth
    from test_nv12_ref import nv12_to_bgr_ref
    sbs, p, H, W = _small_frame(7)
    y, uv = synth.bgr_to_nv12(sbs, 1)
    bgr = np.ascontiguousarray(nv12_to_bgr_ref(y, uv, 1))
    wl, wr, want = frame_lens_ref(orc, bgr, p, (3,) + PANEL, LINEAR_WARP)
    dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    with thread_lens(3, *PANEL):
        dev.d_adcensus_stm_nv12(torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(np.array(uv)).cuda(), dl, dr, out, p,
                                3 | LINEAR_WARP, matrix=1)
        torch.cuda.synchronize()
    assert np.array_equal(dl.cpu().numpy(), wl) and np.array_equal(dr.cpu().numpy(), wr)
    assert np.array_equal(out.cpu().numpy(), want)


def test_reduced_frame_in_mode_3(gpu_ready, orc):
    """stm_adcensus_stm_2s (the host flavour, which ends in the device flavour's render): 40 x 64 matched at 20 x 32, the oracle's
    adcensus_stm_2 maps rendered by render_lens_ref at 50 x 81"""
    from stm_amd import host_api as api
    sbs, p, H, W = _small_frame(3)
    h, w, scale, Ho, Wo = 20, 32, 0.5, 50, 81
    args = (p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    o = orc.adcensus_stm_2(np.array(sbs), Ho, Wo, h, w, scale, *args)
    L, R = orc.demux_sbs(np.array(sbs), W)
    want = render_lens_ref(orc, render_chain(orc, L, R, o["disp_l"], o["disp_r"]), p.num_views, (3,) + PANEL_B, False, Ho, Wo)
    with thread_lens(3, *PANEL_B):
        dl, dr, out = api.adcensus_stm_2s(np.array(sbs), W, Ho, Wo, h, w, scale, *args, stages=3)
    assert np.array_equal(dl, o["disp_l"]) and np.array_equal(dr, o["disp_r"])
    assert np.array_equal(out, want)
    assert np.array_equal(api.adcensus_stm_2s(np.array(sbs), W, Ho, Wo, h, w, scale, *args, stages=3)[2], o["interlaced"])  # mode 0 again


# ----------------------------------------------------------------------------- 3. the frame stream
@pytest.mark.parametrize("temporal", [False, True], ids=["plain", "temporal"])
def test_frame_stream_keeps_its_own_lens(gpu_ready, temporal):
    """stm_stream_set_lens in mode 3, three frames (the third is captured and replayed): each equals the per-frame call under the
    same geometry; the setter refuses after a submit; a thread-level stm_set_lens made between the submits does not reach the
    stream's frames, and the stream's geometry does not reach a plain frame call of the thread"""
    from stm_amd import device_api as dev, synth, video
    H, W, D, zd = 40, 72, 8, 4
    p = _params(D, zd, 9, 4)
    stages = 3 | LINEAR_WARP | (T if temporal else 0)
    frames = [synth.sbs_frame(H, W, D, zd, seed=synth.SEED + 700 + k)[0] for k in range(3)]
    lib = dev.lib()
    plain = _run(frames[0], p, 3)
    fs = video.FrameStream(H, W, p, stages=stages, lens=(3,) + PANEL)
    lib.stm_set_error_mode(1)
    got = []
    try:
        assert fs.submit(frames[0]) == 0
        assert lib.stm_stream_set_lens(fs._h, 1, 8.0, 1.0, 0.0) == -1  # after a submit
        assert b"first submit" in lib.stm_last_error()
        with pytest.raises(ValueError):
            fs.set_lens(0)
        for a, b in zip(plain, _run(frames[0], p, 3)):  # the thread's own frame call, while the stream runs: mode 0
            assert np.array_equal(a, b)
        assert lib.stm_set_lens(1, *PANEL_B) == 0  # the thread's geometry changes under the stream
        assert fs.submit(frames[1]) == 1
        got.append(fs.collect())
        assert fs.submit(frames[2]) == 2
        got.append(fs.collect())
        got.append(fs.collect())
        with_thread_lens = _run(frames[0], p, 3)  # the submits put the thread's mode 1 back
    finally:
        lib.stm_set_error_mode(0)
        lib.stm_set_lens(0, 0.0, 0.0, 0.0)
        fs.close()
    assert [g[0] for g in got] == [0, 1, 2]
    assert not np.array_equal(with_thread_lens[2], plain[2])
    with thread_lens(1, *PANEL_B):
        assert np.array_equal(_run(frames[0], p, 3)[2], with_thread_lens[2])
    hist = None
    with thread_lens(3, *PANEL):
        for k, f in enumerate(frames):
            dl, dr, out = _run_t(f, p, stages, hist) if temporal else _run(f, p, stages)
            assert np.array_equal(got[k][1], dl) and np.array_equal(got[k][2], dr), k
            assert np.array_equal(got[k][3], out), k
            hist = (f, dl, dr)
    assert not np.array_equal(got[0][3], _run(frames[0], p, 3 | LINEAR_WARP)[2])  # and that is not the frame without the lens
    for a, b in zip(plain, _run(frames[0], p, 3)):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- 4. errors
NAN, INF = float("nan"), float("inf")
BAD_GEOMETRY = [(4, 7.37, 0.86, 0.3, b"mode"), (-1, 7.37, 0.86, 0.3, b"mode"), (1, 0.5, 0.86, 0.3, b"pitch"), (2, NAN, 0.86, 0.3, b"pitch"),
                (3, INF, 0.86, 0.3, b"pitch"), (1, 7.37, NAN, 0.3, b"slope"), (2, 7.37, 0.86, INF, b"centre")]


def test_set_lens_refuses_bad_geometry_and_keeps_the_old_one(gpu_ready, orc):
    from stm_amd import device_api as dev, video
    sbs, p, H, W = _small_frame()
    want = frame_lens_ref(orc, sbs, p, (1,) + PANEL)[2]
    lib = dev.lib()
    fs = video.FrameStream(H, W, p)
    lib.stm_set_error_mode(1)
    try:
        assert lib.stm_set_lens(1, *PANEL) == 0
        for mode, pitch, slope, centre, word in BAD_GEOMETRY:
            lib.stm_d_filter_median(None, 0, 0)  # plant a known message
            assert lib.stm_set_lens(mode, pitch, slope, centre) == -1
            err = lib.stm_last_error()
            assert b"set_lens" in err and word in err, err
            assert lib.stm_stream_set_lens(fs._h, mode, pitch, slope, centre) == -1
            err = lib.stm_last_error()
            assert b"stream_set_lens" in err and word in err, err
        assert lib.stm_set_lens(0, NAN, INF, -INF) == 0  # mode 0: the other arguments are ignored
        assert lib.stm_set_lens(1, *PANEL) == 0
        with pytest.raises(ValueError):
            dev.set_lens(4, *PANEL)
        assert np.array_equal(_run(sbs, p, 3)[2], want)  # still the last accepted geometry
    finally:
        lib.stm_set_error_mode(0)
        lib.stm_set_lens(0, 0.0, 0.0, 0.0)
        fs.close()


def test_stage_errors_write_nothing(gpu_ready):
    """mode 0, 3 and 4, a bad pitch / slope / centre, one view, elem_sz 2: reported before anything is launched or written"""
    import torch
    from stm_amd import device_api as dev
    lib = dev.lib()
    N, H, W = 3, 4, 6
    views = random_views(1, N, H, W)
    u8p = C.POINTER(C.c_uint8)
    tab = (u8p * N)(*[v.ctypes.data_as(u8p) for v in views])
    h_out = np.full((H, W, 3), FILL, np.uint8)
    d_views = [torch.from_numpy(v).cuda() for v in views]
    d_tab = torch.tensor([t.data_ptr() for t in d_views], dtype=torch.int64).cuda()
    d_out = torch.full((H, W, 3), FILL, dtype=torch.uint8, device="cuda")
    cases = [(N, 0, 7.37, 0.86, 0.3, 3, b"mode"), (N, 3, 7.37, 0.86, 0.3, 3, b"mode"), (1, 1, 7.37, 0.86, 0.3, 3, b"num_views"),
             (N, 1, 7.37, 0.86, 0.3, 2, b"elem_sz")] + [(N,) + g[:4] + (3, g[4]) for g in BAD_GEOMETRY if g[0] in (1, 2, 4)]
    cases += [(N, 1, 0.5, 0.86, 0.3, 3, b"pitch"), (N, 1, INF, 0.86, 0.3, 3, b"pitch")]
    dev._use_current_stream()
    lib.stm_set_error_mode(1)
    try:
        for n, mode, pitch, slope, centre, e, word in cases:
            lib.stm_d_filter_median(None, 0, 0)
            lib.stm_mux_multiview_lens(C.cast(tab, C.POINTER(u8p)), h_out.ctypes.data_as(u8p), n, mode, pitch, slope, centre, H, W, H, W, e)
            err = lib.stm_last_error()
            assert b"mux_multiview_lens" in err and b"d_mux_multiview_lens" not in err and word in err, (mode, err)
            lib.stm_d_mux_multiview_lens(dev._p(d_tab), dev._p(d_out), n, mode, pitch, slope, centre, H, W, H, W, e)
            torch.cuda.synchronize()
            err = lib.stm_last_error()
            assert b"d_mux_multiview_lens" in err and word in err, (mode, err)
    finally:
        lib.stm_set_error_mode(0)
    assert (h_out == FILL).all() and (d_out.cpu().numpy() == FILL).all()

