"""Overlay at a chosen depth on the GPU (stm_mux_overlay / stm_d_mux_overlay, stm_set_overlay, stm_stream_set_overlay /
stm_stream_overlay), bit for bit against the numpy statement of the definition (test_overlay_ref) -- the stage on random frames and
random premultiplied overlays, the frame calls against the same call with the overlay off, the frame stream with an overlay that
changes between submits, the errors.  Every comparison is over the whole frame.  Every test leaves the thread's overlay, layout, lens
geometry and depth budget at mode 0."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from test_gpu_depth import FILL, _arm, _clean, _frame, _params, _run, thread_depth
from test_gpu_lens import thread_lens
from test_gpu_quilt import thread_layout
from test_lens_ref import LINEAR_WARP
from test_overlay_ref import ANGLE, PANEL, overlay_ref, random_overlay, subpixel_shift_ref, view_coords

pytestmark = pytest.mark.gpu

N = 8


@contextlib.contextmanager
def thread_overlay(d_overlay, x0, y0, disparity):
    """the calling thread's overlay for the duration of the block; off again afterwards, whatever happens"""
    from stm_amd import device_api as dev
    try:
        dev.set_overlay(d_overlay, x0, y0, disparity)
        yield
    finally:
        dev.set_overlay(None)
        assert dev.get_overlay() == (0, 0, 0, 0, 0, 0.0)


_SHIFTS = {}


def _geometry(orc, Ho, Wo, elem_sz, lens=None, layout=None):
    """(shift, coords, (Hv, Wv)) of an output geometry, computed once"""
    key = (Ho, Wo, elem_sz, lens, layout)
    if key not in _SHIFTS:
        Hv, Wv = (Ho, Wo) if layout is None else (Ho // layout[2], Wo // layout[1])
        _SHIFTS[key] = (subpixel_shift_ref(orc, Ho, Wo, N, elem_sz, ANGLE, lens, layout), view_coords(Ho, Wo, N, layout), (Hv, Wv))
    return _SHIFTS[key]


# ----------------------------------------------------------------------------- 1. the stage
GEOMETRIES = {"mux": dict(), "lens1": dict(lens=(1,) + PANEL), "lens2": dict(lens=(2,) + PANEL), "lens3": dict(lens=(3,) + PANEL),
              "quilt4x2_o0": dict(layout=(1, 4, 2, 0)), "quilt4x2_o3": dict(layout=(1, 4, 2, 3)), "quilt2x4_o0": dict(layout=(1, 2, 4, 0)),
              "quilt2x4_o3": dict(layout=(1, 2, 4, 3))}


def _stage_cases(Hv, Wv):
    """((rows, cols), x0, y0, disparity): every overlay size, each side clipped in turn, every disparity"""
    full = (Hv, Wv)
    return [((1, 1), 5, 7, 0.0), ((1, 1), 0, 0, 2.5), ((1, 1), Wv - 1, Hv - 1, -8.0),
            ((3, 5), -2, 3, 8.0), ((3, 5), Wv - 3, 3, -8.0), ((3, 5), 4, -1, 2.5), ((3, 5), 4, Hv - 2, -13.75), ((3, 5), 9, 2, 600.0), ((3, 5), 6, 5, 0.0),
            ((20, 300), -100, 3, 2.5), ((20, 300), -3, -5, -13.75), ((20, 300), 2, Hv - 6, 8.0), ((20, 300), -150, 1, 600.0),
            (full, 0, 0, 0.0), (full, 0, 0, -13.75), (full, 0, 0, 600.0), (full, 1, 1, 8.0), (full, -1, -2, -8.0)]


@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("geom", list(GEOMETRIES), ids=list(GEOMETRIES))
def test_stage_both_flavours(gpu_ready, orc, geom, elem_sz):
    """stm_d_mux_overlay on a frame whose base is 4-byte aligned and on one a byte off, and stm_mux_overlay: the whole frame is the
    statement's -- so the padding bytes and everything outside the bounding box keep their bytes -- and the overlay is read only"""
    import torch
    from stm_amd import device_api as dev, host_api as api
    g = GEOMETRIES[geom]
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    try:
        _arm(lib)
        for Ho, Wo in ((44, 72), (50, 74)):
            shift, coords, (Hv, Wv) = _geometry(orc, Ho, Wo, elem_sz, g.get("lens"), g.get("layout"))
            frame = np.random.RandomState(Ho + elem_sz).randint(0, 256, size=(Ho, Wo, elem_sz)).astype(np.uint8)
            flat = torch.empty(frame.size + 1, dtype=torch.uint8, device="cuda")
            changed = 0
            for k, ((rows, cols), x0, y0, disparity) in enumerate(_stage_cases(Hv, Wv)):
                ov = random_overlay(100 * k + rows, rows, cols)
                d_ov = torch.from_numpy(ov).cuda()
                want = overlay_ref(frame, ov, x0, y0, disparity, shift, coords)
                changed += int(not np.array_equal(want, frame))
                for off in (0, 1):
                    d_frame = flat[off:off + frame.size].view(Ho, Wo, elem_sz)
                    assert d_frame.data_ptr() % 4 == off
                    d_frame.copy_(torch.from_numpy(frame))
                    dev.d_mux_overlay(d_frame, d_ov, x0, y0, disparity, N, ANGLE, g.get("lens"), g.get("layout"))
                    got = d_frame.cpu().numpy()
                    assert np.array_equal(got, want), (Ho, Wo, rows, cols, x0, y0, disparity, off, int((got != want).sum()))
                got = api.mux_overlay(frame, ov, x0, y0, disparity, N, ANGLE, g.get("lens"), g.get("layout"))
                assert np.array_equal(got, want), ("host", Ho, Wo, rows, cols, x0, y0, disparity, int((got != want).sum()))
                assert np.array_equal(d_ov.cpu().numpy(), ov)  # read only
            assert changed >= 12  # the cases are not all empty boxes
        assert _clean(lib)
    finally:
        lib.stm_set_error_mode(0)


@pytest.mark.parametrize("elem_sz", [3, 4])
def test_stage_box_wider_than_a_block(gpu_ready, orc, elem_sz):
    """a block owns 256 columns of 4 rows: a 7 x 600 frame under a 5 x 530 overlay takes three blocks a row and two block rows, the
    last of each partly empty; the reference's interlacer and the continuous lens"""
    import torch
    from stm_amd import device_api as dev
    Ho, Wo = 7, 600
    frame = np.random.RandomState(3).randint(0, 256, size=(Ho, Wo, elem_sz)).astype(np.uint8)
    ov = random_overlay(4, 5, 530)
    d_ov = torch.from_numpy(ov).cuda()
    for lens in (None, (3,) + PANEL):
        shift = subpixel_shift_ref(orc, Ho, Wo, N, elem_sz, ANGLE, lens)
        for x0, disparity in ((33, -13.75), (1, 2.5)):
            d_frame = torch.from_numpy(frame).cuda()
            dev.d_mux_overlay(d_frame, d_ov, x0, 1, disparity, N, ANGLE, lens)
            assert np.array_equal(d_frame.cpu().numpy(), overlay_ref(frame, ov, x0, 1, disparity, shift)), (lens, x0)


# ----------------------------------------------------------------------------- 2. the frame calls
H, W, HO, WO = 40, 64, 44, 72


def _overlays(Hv, Wv):
    """two placements that reach q = -1 and q = ov_cols - 1 inside the view and cross its right and bottom borders"""
    return [(random_overlay(11, 6, 20), -3, 2, 2.5), (random_overlay(12, 5, 9), Wv - 6, Hv - 3, -13.75)]


def _check_frame(orc, run, elem_sz=3, lens=None, layout=None):
    """run() -> (dl, dr, out) with the thread's overlay on equals overlay_ref of the same call with it off; the maps are identical"""
    import torch
    shift, coords, (Hv, Wv) = _geometry(orc, HO, WO, elem_sz, lens, layout)
    dl, dr, base = run()
    for ov, x0, y0, disparity in _overlays(Hv, Wv):
        d_ov = torch.from_numpy(ov).cuda()
        with thread_overlay(d_ov, x0, y0, disparity):
            dl2, dr2, out = run()
        want = overlay_ref(base, ov, x0, y0, disparity, shift, coords)
        assert not np.array_equal(want, base)
        assert np.array_equal(out, want), (x0, y0, disparity, int((out != want).sum()))
        assert np.array_equal(dl2, dl) and np.array_equal(dr2, dr)
        assert np.array_equal(d_ov.cpu().numpy(), ov)


@pytest.mark.parametrize("case", ["plain", "plain_4_byte_pixels", "0x800", "lens3", "depth1", "quilt_area", "agg_variant_200"])
def test_frame_device_flavour(gpu_ready, orc, case):
    from stm_amd import device_api as dev
    sbs, p = _frame(H, W), _params(N)
    elem_sz = 4 if case == "plain_4_byte_pixels" else 3
    stages = 3 | (LINEAR_WARP if case == "0x800" else 0)
    lens = (3,) + PANEL if case == "lens3" else None
    layout = (1, 4, 2, 3) if case == "quilt_area" else None
    with contextlib.ExitStack() as stack:
        if lens:
            stack.enter_context(thread_lens(*lens))
        if layout:
            stack.enter_context(thread_layout(4, 2, 3, 1))
        if case == "depth1":
            stack.enter_context(thread_depth(1, 0.6, 1.5))
        try:
            dev.lib().stm_set_agg_variant(200 if case == "agg_variant_200" else 0)
            _check_frame(orc, lambda: _run(sbs, p, stages, HO, WO, elem_sz), elem_sz, lens, layout)
        finally:
            dev.lib().stm_set_agg_variant(0)


def test_frame_reduced_2s(gpu_ready, orc):
    import torch
    from stm_amd import device_api as dev
    sbs, p = _frame(H, W, 3), _params(N)

    def run():
        dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        dr = torch.zeros_like(dl)
        out = torch.full((HO, WO, 3), FILL, dtype=torch.uint8, device="cuda")
        dev.d_adcensus_stm_2s(torch.from_numpy(np.array(sbs)).cuda(), dl, dr, out, p, 20, 32, 0.5, 3 | 0x1000)
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
        dev.d_adcensus_stm_nv12(torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(np.array(uv)).cuda(), dl, dr, out, p, 3, matrix=1)
        torch.cuda.synchronize()
        return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()
    _check_frame(orc, run)


def test_frame_host_flavour(gpu_ready, orc):
    """stm_adcensus_stm, which ends in the device flavour's render: the overlay stays device memory"""
    from stm_amd import host_api as api
    sbs, p = _frame(H, W), _params(N)
    args = (p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    _check_frame(orc, lambda: api.adcensus_stm(np.array(sbs), W, HO, WO, *args))


def test_a_call_that_renders_nothing_ignores_the_overlay(gpu_ready):
    """stages 2 stops before the renderer: the maps are the plain call's and the output frame is not written"""
    import torch
    from stm_amd import device_api as dev
    sbs, p = _frame(H, W), _params(N)
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    try:
        _arm(lib)
        dl, dr, _ = _run(sbs, p, 2, HO, WO)
        with thread_overlay(torch.from_numpy(random_overlay(1, 6, 20)).cuda(), 3, 2, 2.5):
            dl2, dr2, out = _run(sbs, p, 2, HO, WO)
        assert _clean(lib)
        assert np.array_equal(dl2, dl) and np.array_equal(dr2, dr)
        assert (out == FILL).all()
    finally:
        lib.stm_set_error_mode(0)
    assert dev.get_overlay()[0] == 0


# ----------------------------------------------------------------------------- 3. the frame stream
def _schedule():
    """frame -> the overlay in force when it is submitted: (pixels, x0, y0, disparity) or None"""
    A, B = random_overlay(21, 6, 20), random_overlay(22, 9, 31)
    a0, b0, b1, a1 = (A, 4, 3, 2.5), (B, -5, 15, -8.0), (B, -5, 15, 6.25), (A, 12, -2, -13.75)
    return [a0, a0, b0, b1, None, a1, a1, a1]  # B another size and place; then a new disparity only; none; A elsewhere


def _stream_run(p, frames, stages, schedule, **kw):
    """the frames through a FrameStream, two in flight; schedule None: no overlay at all.  stm_stream_overlay is called only where
    the overlay changes, as a caller would."""
    from stm_amd import video
    fs = video.FrameStream(H, W, p, HO, WO, stages=stages, overlay=None if schedule is None else (16, 40), **kw)
    got = []
    try:
        for k, f in enumerate(frames):
            if k >= 2:
                got.append(fs.collect())
            if schedule is not None and (k == 0 or schedule[k] is not schedule[k - 1]):
                if schedule[k] is None:
                    fs.overlay(None)
                else:
                    pix = np.array(schedule[k][0])
                    fs.overlay(pix, *schedule[k][1:])
                    pix[:] = 0x77  # reusable on return
            assert fs.submit(f) == k
        got.append(fs.collect())
        got.append(fs.collect())
    finally:
        fs.close()
    assert [g[0] for g in got] == list(range(len(frames)))
    return got


@pytest.mark.parametrize("case", ["graphs", "no_graphs", "no_graphs_quilt", "temporal_0x2000"])
def test_stream_overlay_changes_between_submits(gpu_ready, orc, monkeypatch, case):
    """8 frames: both slots replay their captured graphs (from their second frame on) under changed overlays, and frame k shows exactly
    the overlay in force when it was submitted; the maps -- with 0x2000 the history too -- never see it; the calling thread's own
    overlay neither reaches the stream nor is changed by it"""
    import torch
    from stm_amd import device_api as dev
    if case.startswith("no_graphs"):
        monkeypatch.setenv("STM_STREAM_GRAPH", "0")
    stages = 3 | (0x2000 if case == "temporal_0x2000" else 0)
    layout = (1, 4, 2, 3, 1) if case == "no_graphs_quilt" else None
    p = _params(N)
    frames = [_frame(H, W, 40 + k) for k in range(8)]
    schedule = _schedule()
    mine = torch.from_numpy(random_overlay(23, 4, 4)).cuda()
    with thread_overlay(mine, 1, 1, 3.0):
        base = _stream_run(p, frames, stages, None, layout=layout)
        got = _stream_run(p, frames, stages, schedule, layout=layout)
        assert dev.get_overlay() == (1, 4, 4, 1, 1, 3.0)
    shift, coords, _ = _geometry(orc, HO, WO, 3, None, None if layout is None else layout[:4])
    differ = 0
    for k in range(8):
        want = base[k][3] if schedule[k] is None else overlay_ref(base[k][3], schedule[k][0], *schedule[k][1:], shift, coords)
        differ += int(not np.array_equal(want, base[k][3]))
        assert np.array_equal(got[k][3], want), (k, int((got[k][3] != want).sum()))
        assert np.array_equal(got[k][1], base[k][1]) and np.array_equal(got[k][2], base[k][2]), k
    assert differ == 7
    if layout is None and stages == 3:  # the thread's overlay did not reach the stream: frame 0 is the plain frame call's
        assert np.array_equal(base[0][3], _run(frames[0], p, 3, HO, WO)[2])


# ----------------------------------------------------------------------------- 4. errors
def test_stage_refusals_leave_the_frame_alone(gpu_ready):
    import torch
    from stm_amd import device_api as dev
    lib = dev.lib()
    frame = torch.full((HO, WO, 3), FILL, dtype=torch.uint8, device="cuda")
    ov = torch.from_numpy(random_overlay(1, 3, 5)).cuda()
    good = (N, ANGLE, 0, 0.0, 0.0, 0.0, 0, 1, 1, 0, HO, WO, 3)
    lib.stm_set_error_mode(1)
    try:
        for args, word in (((0, 5, 0, 0, 0.0) + good, b"ov_rows"), ((3, 5, 0, 0, float("nan")) + good, b"disparity"),
                           ((3, 5, 1 << 17, 0, 0.0) + good, b"x0"), ((3, 5, 0, 0, 0.0) + good[:6] + (1, 4, 3, 0, HO, WO, 3), b"num_views"),
                           ((3, 5, 0, 0, 0.0) + (N, 0.0) + good[2:], b"angle")):
            _arm(lib)
            lib.stm_d_mux_overlay(frame.data_ptr(), ov.data_ptr(), *args)
            assert word in lib.stm_last_error(), args
        _arm(lib)
        lib.stm_d_mux_overlay(frame.data_ptr(), ov.data_ptr() + 1, 3, 4, 0, 0, 0.0, *good)
        assert b"aligned" in lib.stm_last_error()
        torch.cuda.synchronize()
        assert (frame.cpu().numpy() == FILL).all()
    finally:
        lib.stm_set_error_mode(0)


def test_frame_call_refuses_nv12_output_in_both_orders(gpu_ready):
    import torch
    from stm_amd import device_api as dev
    sbs, p = _frame(H, W), _params(N)
    lib = dev.lib()
    d_ov = torch.from_numpy(random_overlay(1, 3, 5)).cuda()
    d_sbs = torch.from_numpy(np.array(sbs)).cuda()
    lib.stm_set_error_mode(1)
    try:
        for overlay_first in (True, False):
            with thread_layout(4, 2, 0, 1):
                try:
                    steps = [lambda: dev.set_overlay(d_ov, 1, 1, 2.0), lambda: dev.set_output(1, 0)]
                    for step in (steps if overlay_first else steps[::-1]):
                        step()
                    _arm(lib)
                    dl = torch.full((H, W), float(FILL), dtype=torch.float32, device="cuda")
                    dr = torch.full_like(dl, float(FILL))
                    out = torch.full((48 * 3 // 2, 72), FILL, dtype=torch.uint8, device="cuda")  # the NV12 surface of a 48 x 72 quilt
                    lib.stm_d_adcensus_stm(d_sbs.data_ptr(), dl.data_ptr(), dr.data_ptr(), out.data_ptr(), H, 2 * W, W, 48, 72, 3, p.num_views,
                                           p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s,
                                           p.thresh_h, 3)
                    torch.cuda.synchronize()
                    dl, dr, out = dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()
                    err = lib.stm_last_error()
                    assert b"d_adcensus_stm:" in err and b"overlay" in err and b"NV12" in err, err
                    assert (out == FILL).all() and (dl == FILL).all() and (dr == FILL).all()
                    assert dev.get_overlay() == (1, 3, 5, 1, 1, 2.0) and dev.get_output() == (1, 0, 0, 0)
                finally:
                    dev.set_output(0)
                    dev.set_overlay(None)
    finally:
        lib.stm_set_error_mode(0)


def test_stream_refusals(gpu_ready):
    from stm_amd import device_api as dev, video
    lib = dev.lib()
    p = _params(N)
    ov = random_overlay(1, 6, 20)
    u8p = C.POINTER(C.c_uint8)
    lib.stm_set_error_mode(1)
    try:
        fs = video.FrameStream(H, W, p, HO, WO)
        try:
            _arm(lib)
            with pytest.raises(ValueError, match="stm_stream_set_overlay"):  # no overlay was ever set up
                fs.overlay(ov, 1, 1, 0.0)
            for args in ((0, 5), (5, 0), (65536, 5), (5, 65536), (-1, -1)):
                with pytest.raises(ValueError, match="max_rows"):
                    fs.set_overlay(*args)
            fs.set_overlay(6, 20)
            fs.set_overlay(0, 0)  # off again
            with pytest.raises(ValueError, match="stm_stream_set_overlay"):
                fs.overlay(ov, 1, 1, 0.0)
            fs.set_overlay(6, 20)
            for shape, word in (((7, 20), "at most 6 x 20"), ((6, 21), "at most 6 x 20")):
                with pytest.raises(ValueError, match=word):
                    fs.overlay(np.zeros(shape + (4,), np.uint8), 0, 0, 0.0)
            for args, word in (((1 << 17, 0, 0.0), "x0"), ((0, -(1 << 17), 0.0), "y0"), ((0, 0, float("inf")), "disparity"), ((0, 0, 5000.0), "disparity")):
                with pytest.raises(ValueError, match=word):
                    fs.overlay(ov, *args)
            assert lib.stm_stream_overlay(fs._h, ov.ctypes.data_as(u8p), 0, 20, 0, 0, 0.0) == 0  # a zero size: no overlay
            # NV12 output, refused in both orders
            fs.set_layout(1, 4, 2, 0, 1)
            with pytest.raises(ValueError, match="overlay"):
                fs.set_output(1, 0)
            fs.set_overlay(0, 0)
            fs.set_output(1, 0)
            with pytest.raises(ValueError, match="NV12"):
                fs.set_overlay(6, 20)
            fs.set_output(0, 0)
            fs.set_layout(0)
            fs.set_overlay(6, 20)
            fs.overlay(ov[:, 1:], 2, 3, 1.0)
            assert fs.submit(_frame(H, W)) == 0
            with pytest.raises(ValueError, match="first submit"):
                fs.set_overlay(8, 8)
            out = fs.collect()[3]
            assert not (out == 0).all()
        finally:
            fs.close()
    finally:
        lib.stm_set_error_mode(0)
    assert dev.get_overlay()[0] == 0
