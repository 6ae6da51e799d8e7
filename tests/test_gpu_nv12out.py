"""NV12 output on the GPU (stm_set_output, stm_mux_nv12 / stm_d_mux_nv12, stm_stream_set_output), bit for bit against
bgr_to_nv12_ref (test_nv12out_ref) of the existing numpy statements of the quilt (test_quilt_ref): the stage on random images, the
frame calls on the oracle's chain, the frame stream, the errors.  Every test leaves the thread's format at 0, its layout, lens geometry
and depth budget at mode 0 and the staging limit at its default."""
import contextlib
import copy
import ctypes as C
import threading

import numpy as np
import pytest

from test_depth_ref import depth_fit_ref
from test_gpu_depth import AUTO, FILL, _arm, _chain_of, _clean, _frame, _pad, _params, _run, thread_depth
from test_gpu_quilt import thread_layout
from test_lens_ref import LINEAR_WARP, frame_chain
from test_nv12out_ref import bgr_to_nv12_ref, nv12_surface_ref, random_image
from test_quilt_ref import render_quilt_ref

pytestmark = pytest.mark.gpu

f32 = np.float32


@contextlib.contextmanager
def thread_output(matrix, pitch=0, uv_row=0):
    """the calling thread's format 1 for the duration of the block; BGR again afterwards"""
    from stm_amd import device_api as dev
    try:
        dev.set_output(1, matrix, pitch, uv_row)
        yield
    finally:
        assert dev.lib().stm_set_output(0, 0, 0, 0) == 0


# ----------------------------------------------------------------------------- 1. the stage
# 2 x 6: a width that is no multiple of 4; 4 x 258 and 6 x 1026 cross a 256-thread block at one, two and four columns a thread
STAGE_SHAPES = [(2, 2), (2, 6), (4, 258), (6, 1026)]


@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_stage_both_flavours(gpu_ready, shape, elem_sz):
    """stm_d_mux_nv12 and stm_mux_nv12, the four matrices, pitches W and W + 3, both plane bases one byte off: the samples are the
    statement's, every other byte keeps its fill from the device flavour and comes back 0 from the host flavour, img is read only"""
    import torch
    from stm_amd import device_api as dev, host_api as api
    H, W = shape
    img = random_image(H * 31 + W + elem_sz, H, W, elem_sz)
    d_img = torch.from_numpy(img).cuda()
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    try:
        _arm(lib)
        for matrix in range(4):
            wy, wuv = bgr_to_nv12_ref(img, matrix)
            for pitch in (W, W + 3):
                for off in (0, 1):
                    by = torch.full((off + H * pitch,), FILL, dtype=torch.uint8, device="cuda")
                    buv = torch.full((off + (H // 2) * pitch,), FILL, dtype=torch.uint8, device="cuda")
                    y, uv = by[off:].view(H, pitch), buv[off:].view(H // 2, pitch)
                    assert y.data_ptr() % 2 == off or off == 0
                    dev.d_mux_nv12(y, uv, d_img, matrix)
                    gy, guv = by.cpu().numpy(), buv.cpu().numpy()
                    assert (gy[:off] == FILL).all() and (guv[:off] == FILL).all()
                    gy, guv = gy[off:].reshape(H, pitch), guv[off:].reshape(H // 2, pitch)
                    assert np.array_equal(gy[:, :W], wy), (matrix, pitch, off, int((gy[:, :W] != wy).sum()))
                    assert np.array_equal(guv[:, :W], wuv), (matrix, pitch, off, int((guv[:, :W] != wuv).sum()))
                    assert (gy[:, W:] == FILL).all() and (guv[:, W:] == FILL).all()
                hy, huv = api.mux_nv12(img, matrix, pitch, pitch)
                assert np.array_equal(hy[:, :W], wy) and np.array_equal(huv[:, :W], wuv), ("host", matrix, pitch)
                assert (hy[:, W:] == 0).all() and (huv[:, W:] == 0).all()
        assert _clean(lib)
        assert np.array_equal(d_img.cpu().numpy(), img)  # read only
    finally:
        lib.stm_set_error_mode(0)


# ----------------------------------------------------------------------------- 2. the frame
H, W = 40, 64
# (tiles_x, tiles_y), (Ho, Wo): 18 x 22 tiles with fractional footprints (18 is no multiple of 4); two remainder columns; two remainder rows
GEOMETRIES = {"44x72": ((4, 2), (44, 72)), "48x74_remainder_columns": ((4, 2), (48, 74)), "50x72_remainder_rows": ((2, 4), (50, 72))}
_WANT = {}


def _want(orc, ch, N, tiles, order, filter, Ho, Wo, linear, matrix, depth=None, key=None):
    """the NV12 surface of the statement's quilt, computed once per case"""
    k = (key, N, tiles, order, filter, Ho, Wo, linear, matrix, depth)
    if key is None or k not in _WANT:
        quilt = render_quilt_ref(orc, ch, N, tiles[0], tiles[1], order, filter, Ho, Wo, linear, depth=depth)
        s = nv12_surface_ref(quilt, matrix)
        s.setflags(write=False)
        if key is None:
            return s
        _WANT[k] = s
    return _WANT[k]


def _run_nv12(sbs, p, stages, Ho, Wo, elem_sz=3, pitch=0, uv_row=0):
    """d_adcensus_stm into an NV12 surface under the thread's format: (disp_l, disp_r, surface uint8 [R + Ho / 2][P])"""
    import torch
    from stm_amd import device_api as dev
    Hh, Ww = sbs.shape[0], sbs.shape[1] // 2
    d_sbs = torch.from_numpy(_pad(sbs, elem_sz)).cuda()
    dl = torch.full((Hh, Ww), float(FILL), dtype=torch.float32, device="cuda")
    dr = torch.full_like(dl, float(FILL))
    out = torch.full(((uv_row or Ho) + Ho // 2, pitch or Wo), FILL, dtype=torch.uint8, device="cuda")
    q = copy.copy(p)
    q.out_rows, q.out_cols = Ho, Wo
    dev.d_adcensus_stm(d_sbs, dl, dr, out, q, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _check_maps(ch, dl, dr):
    assert np.array_equal(dl, ch["dl"]) and np.array_equal(dr, ch["dr"])  # the format does not reach the maps


@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("geom", list(GEOMETRIES), ids=list(GEOMETRIES))
def test_frame_nv12_both_filters(gpu_ready, orc, geom, elem_sz):
    """stm_d_adcensus_stm under layout 1 and format 1, 8 views: both filters, orders 0 and 3; the area filter with every staging
    limit (64: the per-block form); stm_set_agg_variant(200) -- the BGR quilt in the workspace, then stm_k_mux_nv12 -- gives the
    same bytes; the maps are the BGR call's"""
    from stm_amd import device_api as dev
    tiles, (Ho, Wo) = GEOMETRIES[geom]
    N, matrix = 8, {3: 0, 4: 3}[elem_sz]
    sbs, p = _frame(H, W), _params(N)
    ch = frame_chain(orc, sbs, p, 0)
    lib = dev.lib()
    seen = set()
    for order in (0, 3):
        for filter in (0, 1):
            want = _want(orc, ch, N, tiles, order, filter, Ho, Wo, False, matrix, key="frame0")
            with thread_layout(tiles[0], tiles[1], order, filter):
                bgr = _run(sbs, p, 3, Ho, Wo, elem_sz)
                with thread_output(matrix):
                    for limit in ((0, 2048, 64) if filter == 1 else (0,)):
                        lib.stm_set_quilt_lds_limit(limit)
                        dl, dr, out = _run_nv12(sbs, p, 3, Ho, Wo, elem_sz)
                        _check_maps(ch, dl, dr)
                        assert np.array_equal(dl, bgr[0]) and np.array_equal(dr, bgr[1])
                        assert np.array_equal(out, want), (order, filter, limit, int((out != want).sum()))
                    lib.stm_set_quilt_lds_limit(0)
                    lib.stm_set_agg_variant(200)
                    unfused = _run_nv12(sbs, p, 3, Ho, Wo, elem_sz)[2]
                    lib.stm_set_agg_variant(0)
                    assert np.array_equal(unfused, out), (order, filter)
                # ... and it is the conversion of the bytes the BGR call stores
                assert np.array_equal(out, nv12_surface_ref(bgr[2], matrix)), (order, filter)
            seen.add(out.tobytes())
    assert len(seen) == 4


@pytest.mark.parametrize("filter", [0, 1])
def test_frame_nv12_linear_warp_and_padded_surface(gpu_ready, orc, filter):
    """0x800, and a surface with P = Wout + 5, R = Hout + 3 whose bytes outside the samples keep their fill"""
    tiles, (Ho, Wo) = GEOMETRIES["44x72"]
    N, matrix = 8, 1
    sbs, p = _frame(H, W), _params(N)
    ch = frame_chain(orc, sbs, p, LINEAR_WARP)
    want = _want(orc, ch, N, tiles, 3, filter, Ho, Wo, True, matrix)
    assert not np.array_equal(want, _want(orc, ch, N, tiles, 3, filter, Ho, Wo, False, matrix, key="frame0"))
    with thread_layout(tiles[0], tiles[1], 3, filter):
        with thread_output(matrix):
            dl, dr, out = _run_nv12(sbs, p, 3 | LINEAR_WARP, Ho, Wo)
        _check_maps(ch, dl, dr)
        assert np.array_equal(out, want), int((out != want).sum())
        P, R = Wo + 5, Ho + 3
        with thread_output(matrix, P, R):
            dl, dr, out = _run_nv12(sbs, p, 3 | LINEAR_WARP, Ho, Wo, pitch=P, uv_row=R)
        _check_maps(ch, dl, dr)
        padded = np.full((R + Ho // 2, P), FILL, np.uint8)
        padded[:Ho, :Wo] = want[:Ho]
        padded[R:, :Wo] = want[Ho:]
        assert np.array_equal(out, padded), int((out != padded).sum())


@pytest.mark.parametrize("stages", [3, 3 | LINEAR_WARP], ids=["0x3", "0x803"])
def test_frame_nv12_with_manual_depth(gpu_ready, orc, stages):
    """depth mode 1 (0.6, 1.5), both filters, the per-block form and 200 (no views to write: the fused kernels)"""
    from stm_amd import device_api as dev
    tiles, (Ho, Wo) = GEOMETRIES["48x74_remainder_columns"]
    N, matrix = 8, 2
    sbs, p = _frame(H, W), _params(N)
    ch = frame_chain(orc, sbs, p, 0)
    linear = bool(stages & LINEAR_WARP)
    lib = dev.lib()
    for filter in (0, 1):
        want = _want(orc, ch, N, tiles, 1, filter, Ho, Wo, linear, matrix, depth=(0.6, 1.5))
        with thread_layout(tiles[0], tiles[1], 1, filter), thread_depth(1, 0.6, 1.5), thread_output(matrix):
            for limit, variant in ((0, 0), (64, 0), (0, 200)):
                lib.stm_set_quilt_lds_limit(limit)
                lib.stm_set_agg_variant(variant)
                dl, dr, out = _run_nv12(sbs, p, stages, Ho, Wo)
                _check_maps(ch, dl, dr)
                assert np.array_equal(out, want), (filter, limit, variant, int((out != want).sum()))


def test_frame_nv12_with_automatic_depth(gpu_ready, orc):
    """depth mode 2: the state's four floats are the same with and without the format, and the surface is rendered with them"""
    import torch
    from stm_amd import device_api as dev
    tiles, (Ho, Wo) = GEOMETRIES["50x72_remainder_rows"]
    N, matrix = 8, 0
    sbs, p = _frame(H, W, 30), _params(N)
    lo, hi, mg, clip = AUTO
    lib = dev.lib()
    try:
        plain = torch.zeros(4, dtype=torch.float32, device="cuda")
        dev.set_depth_auto(lo, hi, mg, clip, 1.0, plain)
        with thread_layout(tiles[0], tiles[1], 2, 1), thread_depth(2):
            dl, dr, _ = _run(sbs, p, 3, Ho, Wo)
        want_st = depth_fit_ref(dl, dr, lo, hi, mg, clip, 1.0, np.zeros(4, f32))
        assert plain.cpu().numpy().tobytes() == want_st.tobytes()
        ch = _chain_of(orc, sbs, dl, dr)
        for filter in (0, 1):
            state = torch.zeros(4, dtype=torch.float32, device="cuda")
            dev.set_depth_auto(lo, hi, mg, clip, 1.0, state)
            with thread_layout(tiles[0], tiles[1], 2, filter), thread_depth(2), thread_output(matrix):
                dl2, dr2, out = _run_nv12(sbs, p, 3, Ho, Wo)
            assert np.array_equal(dl2, dl) and np.array_equal(dr2, dr)
            assert state.cpu().numpy().tobytes() == want_st.tobytes(), filter
            want = _want(orc, ch, N, tiles, 2, filter, Ho, Wo, False, matrix, depth=(float(want_st[1]), float(want_st[2])))
            assert np.array_equal(out, want), (filter, int((out != want).sum()))
    finally:
        lib.stm_set_depth(0, 0.0, 0.0)
        lib.stm_set_depth_auto(-1.0, 1.0, 1.0, 20, 1.0, None)  # drop the pointer to this test's tensors


def test_retargeted_stereo_pair_nv12(gpu_ready, orc):
    """num_views 2 as 2 x 1 tiles, order 2, at 40 x 152 with a depth budget: what a stereo encoder takes"""
    Ho, Wo, N, matrix = 40, 152, 2, 1
    sbs, p = _frame(H, W), _params(N)
    ch = frame_chain(orc, sbs, p, 0)
    for filter in (0, 1):
        want = _want(orc, ch, N, (2, 1), 2, filter, Ho, Wo, False, matrix, depth=(0.5, -1.0))
        with thread_layout(2, 1, 2, filter), thread_depth(1, 0.5, -1.0), thread_output(matrix):
            dl, dr, out = _run_nv12(sbs, p, 3, Ho, Wo)
        _check_maps(ch, dl, dr)
        assert np.array_equal(out, want), (filter, int((out != want).sum()))


def test_other_frame_entries(gpu_ready, orc):
    """_t, NV12 input, _2s with 0x1000, and the host flavour (whose bytes outside the samples come back 0)"""
    import torch
    from stm_amd import device_api as dev, host_api as api, synth
    from test_nv12_ref import nv12_to_bgr_ref
    tiles, (Ho, Wo) = GEOMETRIES["44x72"]
    N, matrix = 8, 3
    sbs, p = _frame(H, W, 3), _params(N)
    ch = frame_chain(orc, sbs, p, 0)
    d_sbs = torch.from_numpy(np.array(sbs)).cuda()

    def outputs():
        dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        return dl, torch.zeros_like(dl), torch.full((Ho * 3 // 2, Wo), FILL, dtype=torch.uint8, device="cuda")
    with thread_layout(tiles[0], tiles[1], 3, 1), thread_output(matrix):
        want = _want(orc, ch, N, tiles, 3, 1, Ho, Wo, False, matrix)
        dl, dr, out = outputs()
        dev.d_adcensus_stm_t(d_sbs, dl, dr, out, p, 3)  # no history: the first frame of a sequence
        torch.cuda.synchronize()
        _check_maps(ch, dl.cpu().numpy(), dr.cpu().numpy())
        assert np.array_equal(out.cpu().numpy(), want)
        # the host flavour, a padded surface: Y rows, three rows of 0, UV rows; five bytes of 0 behind every row
        args = (p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
        dev.set_output(1, matrix, Wo + 5, Ho + 3)
        hl, hr, hout = api.adcensus_stm(np.array(sbs), W, Ho, Wo, *args)
        dev.set_output(1, matrix)
        _check_maps(ch, hl, hr)
        padded = np.zeros((Ho + 3 + Ho // 2, Wo + 5), np.uint8)
        padded[:Ho, :Wo] = want[:Ho]
        padded[Ho + 3:, :Wo] = want[Ho:]
        assert hout.shape == padded.shape and np.array_equal(hout, padded)
        # the reduced-resolution frame with the guided up-sampler: rendered from the maps the call returns
        dl, dr, out = outputs()
        dev.d_adcensus_stm_2s(d_sbs, dl, dr, out, p, 20, 32, 0.5, 3 | 0x1000)
        torch.cuda.synchronize()
        ch2 = _chain_of(orc, sbs, dl.cpu().numpy(), dr.cpu().numpy())
        assert np.array_equal(out.cpu().numpy(), _want(orc, ch2, N, tiles, 3, 1, Ho, Wo, False, matrix))
        # NV12 in, NV12 out
        y, uv = synth.bgr_to_nv12(sbs, 1)
        bgr = np.ascontiguousarray(nv12_to_bgr_ref(y, uv, 1))
        ch3 = frame_chain(orc, bgr, p, 0)
        dl, dr, out = outputs()
        dev.d_adcensus_stm_nv12(torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(np.array(uv)).cuda(), dl, dr, out, p, 3, matrix=1)
        torch.cuda.synchronize()
        _check_maps(ch3, dl.cpu().numpy(), dr.cpu().numpy())
        assert np.array_equal(out.cpu().numpy(), _want(orc, ch3, N, tiles, 3, 1, Ho, Wo, False, matrix))


def test_a_call_that_renders_nothing_ignores_the_format(gpu_ready, orc):
    """stages 2 stops before the renderer: format 1 under layout 0, which a rendering call refuses, is no error there"""
    from stm_amd import device_api as dev
    sbs, p = _frame(H, W), _params(8)
    ch = frame_chain(orc, sbs, p, 0)
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    try:
        _arm(lib)
        with thread_output(0):
            dl, dr, out = _run_nv12(sbs, p, 2, 44, 72)
        assert _clean(lib)
        _check_maps(ch, dl, dr)
        assert (out == FILL).all()
    finally:
        lib.stm_set_error_mode(0)


# ----------------------------------------------------------------------------- 3. the frame stream
def _stream_case(fs_kwargs, frames, per_frame, Ho, Wo):
    """four frames through a stream (the third and fourth replay the captured graphs) against per_frame(k) -> (dl, dr, surface)"""
    from stm_amd import device_api as dev, video
    lib = dev.lib()
    fs = video.FrameStream(H, W, _params(8), Ho, Wo, **fs_kwargs)
    lib.stm_set_error_mode(1)
    got = []
    try:
        assert dev.get_output() == (0, 0, 0, 0)
        assert fs.submit(frames[0]) == 0
        assert lib.stm_stream_set_output(fs._h, 0, 0) == -1 and b"first submit" in lib.stm_last_error()
        assert fs.submit(frames[1]) == 1
        got.append(fs.collect())
        assert fs.submit(frames[2]) == 2
        got.append(fs.collect_view())
        got[-1] = tuple(np.array(a) if isinstance(a, np.ndarray) else a for a in got[-1])
        assert fs.submit(frames[3]) == 3
        got.append(fs.collect())
        got.append(fs.collect())
        assert dev.get_output() == (0, 0, 0, 0)  # the thread's own format is untouched
    finally:
        fs.close()
        lib.stm_set_error_mode(0)
    for k, (idx, dl, dr, out) in enumerate(got):
        assert idx == k and out.shape == (Ho * 3 // 2, Wo) and out.nbytes == Ho * Wo * 3 // 2
        want = per_frame(k)
        assert np.array_equal(dl, want[0]) and np.array_equal(dr, want[1]) and np.array_equal(out, want[2]), k


def test_stream_output_is_the_frame_call(gpu_ready):
    tiles, (Ho, Wo) = GEOMETRIES["44x72"]
    p = _params(8)
    frames = [_frame(H, W, 20 + k) for k in range(4)]

    def per_frame(k):
        with thread_layout(tiles[0], tiles[1], 3, 1), thread_output(1):
            return _run_nv12(frames[k], p, 3 | LINEAR_WARP, Ho, Wo)
    _stream_case(dict(stages=3 | LINEAR_WARP, layout=(1,) + tiles + (3, 1), output=(1, 1)), frames, per_frame, Ho, Wo)


def test_stream_nv12_in_nv12_out_with_a_match_size(gpu_ready):
    import torch
    from stm_amd import device_api as dev, synth
    from test_nv12_ref import nv12_frame
    tiles, (Ho, Wo) = GEOMETRIES["48x74_remainder_columns"]
    p = _params(8)
    planes = [synth.bgr_to_nv12(_frame(H, W, 40 + k), 0) for k in range(4)]

    def per_frame(k):
        y, uv = (torch.from_numpy(np.array(a)).cuda() for a in planes[k])
        dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        dr = torch.zeros_like(dl)
        out = torch.full((Ho * 3 // 2, Wo), FILL, dtype=torch.uint8, device="cuda")
        with thread_layout(tiles[0], tiles[1], 0, 0), thread_output(2):
            dev.d_adcensus_stm_2nv12(y, uv, dl, dr, out, p, 20, 32, 0.5, 3, matrix=0)
            torch.cuda.synchronize()
        return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()
    _stream_case(dict(input_format="nv12", matrix=0, layout=(1,) + tiles + (0, 0), output=(1, 2), match=(20, 32, 0.5)),
                 [nv12_frame(*pl) for pl in planes], per_frame, Ho, Wo)


def test_stream_output_ordering_rules(gpu_ready):
    """refused while the stream's layout is 0; the layout cannot go back to 0 while the format is 1; both directions leave the stream as
    it was"""
    from stm_amd import device_api as dev, video
    lib = dev.lib()
    fs = video.FrameStream(H, W, _params(8), 44, 72)
    lib.stm_set_error_mode(1)
    try:
        assert lib.stm_stream_set_output(fs._h, 1, 0) == -1
        err = lib.stm_last_error()
        assert b"stream_set_output" in err and b"layout" in err, err
        for bad, word in (((2, 0), b"format"), ((1, 4), b"matrix"), ((-1, 0), b"format")):
            assert lib.stm_stream_set_output(fs._h, *bad) == -1 and word in lib.stm_last_error()
        assert lib.stm_stream_set_output(fs._h, 0, 7) == 0  # format 0: the matrix is ignored
        assert lib.stm_stream_set_layout(fs._h, 1, 4, 2, 0, 1) == 0
        assert lib.stm_stream_set_output(fs._h, 1, 3) == 0
        assert lib.stm_stream_set_layout(fs._h, 0, 0, 0, 0, 0) == -1
        err = lib.stm_last_error()
        assert b"stream_set_layout" in err and b"NV12" in err, err
        assert lib.stm_stream_set_layout(fs._h, 1, 2, 4, 3, 0) == 0  # another quilt is fine
        assert lib.stm_stream_set_output(fs._h, 0, 0) == 0
        assert lib.stm_stream_set_layout(fs._h, 0, 0, 0, 0, 0) == 0
        with pytest.raises(ValueError):
            fs.set_output(1, 0)
        assert fs.out_shape == (44, 72, 3)
    finally:
        fs.close()
        lib.stm_set_error_mode(0)


# ----------------------------------------------------------------------------- 4. errors
def test_frame_errors_launch_nothing_and_name_the_argument(gpu_ready):
    """each refusal of a frame call under format 1 leaves the maps and a generous surface with their fill.  The C call is made
    directly: the Python wrapper would not let a surface through whose shape contradicts the format."""
    import torch
    from stm_amd import device_api as dev
    sbs, p = _frame(H, W), _params(8)
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    # (layout or None, (pitch, uv_row), (Ho, Wo), the words)
    cases = [(None, (0, 0), (44, 72), (b"quilts only",)), ((4, 2, 0, 1), (0, 0), (45, 72), (b"num_rows_out", b"even")),
             ((4, 2, 0, 0), (0, 0), (44, 73), (b"num_cols_out", b"even")), ((4, 2, 0, 1), (0, 0), (46, 72), (b"tile height",)),
             ((4, 2, 0, 0), (0, 0), (44, 76), (b"tile width",)), ((4, 2, 0, 1), (71, 0), (44, 72), (b"pitch",)),
             ((4, 2, 0, 0), (0, 43), (44, 72), (b"uv_row",))]
    d_sbs = torch.from_numpy(np.array(sbs)).cuda()
    try:
        for lo, (pitch, uv_row), (Ho, Wo), words in cases:
            dl = torch.full((H, W), float(FILL), dtype=torch.float32, device="cuda")
            dr = torch.full_like(dl, float(FILL))
            out = torch.full((2 * Ho, Wo + 8), FILL, dtype=torch.uint8, device="cuda")
            _arm(lib)
            with (thread_layout(*lo) if lo else contextlib.nullcontext()), thread_output(1, pitch, uv_row):
                lib.stm_d_adcensus_stm(C.c_void_p(d_sbs.data_ptr()), C.c_void_p(dl.data_ptr()), C.c_void_p(dr.data_ptr()),
                                       C.c_void_p(out.data_ptr()), H, 2 * W, W, Ho, Wo, 3, p.num_views, p.angle, p.num_disp, p.zero_disp,
                                       p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, 3)
                torch.cuda.synchronize()
            err = lib.stm_last_error()
            assert b"d_adcensus_stm:" in err and all(w in err for w in words), (lo, err)
            assert (out.cpu().numpy() == FILL).all() and (dl.cpu().numpy() == FILL).all() and (dr.cpu().numpy() == FILL).all(), lo
    finally:
        lib.stm_set_error_mode(0)


# ----------------------------------------------------------------------------- 5. the default
def test_format_0_is_the_frame_of_a_fresh_thread(gpu_ready):
    """format 0 set explicitly, after an NV12 surface was rendered on this thread, gives the bytes a thread that never set one gets"""
    from stm_amd import device_api as dev
    sbs, p = _frame(H, W), _params(8)
    with thread_layout(4, 2, 3, 1):
        with thread_output(1):
            _run_nv12(sbs, p, 3, 44, 72)
        dev.set_output(0, 3, 99, 99)
        assert dev.get_output() == (0, 0, 0, 0)
        quilt = _run(sbs, p, 3, 44, 72)
    here = _run(sbs, p, 3, 44, 72)
    box = {}

    def fresh():
        box["output"] = dev.get_output()
        box["out"] = _run(sbs, p, 3, 44, 72)
        dev.set_layout(1, 4, 2, 3, 1)
        box["quilt"] = _run(sbs, p, 3, 44, 72)
        dev.set_layout(0)
        dev.lib().stm_release_workspace()

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert box["output"] == (0, 0, 0, 0)
    for a, b in zip(here, box["out"]):
        assert np.array_equal(a, b)
    for a, b in zip(quilt, box["quilt"]):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- 6. the tool
def test_video_cli_nv12_out(gpu_ready, tmp_path):
    """tools/stm_video.py --quilt 4 2 3 1 --nv12-out 1 on a directory of BMP frames: quilt.yuv holds the per-frame calls' surfaces"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from stm_amd import bmp_io
    Ho, Wo = 44, 72
    p = _params(8)
    frames = [_frame(H, W, 50 + k) for k in range(3)]
    for k, f in enumerate(frames):
        bmp_io.write_bmp(str(tmp_path / ("f%03d.bmp" % k)), np.array(f))
    out = tmp_path / "o"
    args = [sys.executable, os.path.join(ROOT, "tools", "stm_video.py"), str(tmp_path), "8", "18.43", str(Wo), str(Ho), str(p.num_disp),
            str(p.zero_disp), str(p.ad_coeff), str(p.census_coeff), str(p.ucd), str(p.lcd), str(p.usd), str(p.lsd), str(p.thresh_s),
            str(p.thresh_h), str(out), "--quilt", "4", "2", "3", "1", "--nv12-out", "1"]
    subprocess.check_call(args)
    assert sorted(os.listdir(out)) == sorted(["quilt.yuv"] + ["%s_%05d.bmp" % (n, k) for n in ("disp_l", "disp_r") for k in range(3)])
    got = np.fromfile(str(out / "quilt.yuv"), np.uint8).reshape(3, Ho * 3 // 2, Wo)
    for k, f in enumerate(frames):
        with thread_layout(4, 2, 3, 1), thread_output(1):
            assert np.array_equal(got[k], _run_nv12(f, p, 3, Ho, Wo)[2]), k
