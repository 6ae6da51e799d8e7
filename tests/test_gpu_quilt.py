"""Quilt output on the GPU (stm_set_layout, stm_quilt_multiview / stm_d_quilt_multiview, stm_stream_set_layout), bit for bit against the
numpy statement of the definition (test_quilt_ref) -- the stage on random views, the frame calls on the oracle's chain, the frame
stream, the errors.  Every test leaves the thread's layout, lens geometry and depth budget at mode 0 and the staging limit at its
default."""
import contextlib
import ctypes as C
import threading

import numpy as np
import pytest

from test_depth_ref import depth_fit_ref
from test_gpu_depth import AUTO, FILL, _arm, _chain_of, _clean, _frame, _params, _run, thread_depth
from test_lens_ref import LINEAR_WARP, frame_chain, random_views
from test_quilt_ref import quilt_ref, render_quilt_ref

pytestmark = pytest.mark.gpu

f32 = np.float32


@contextlib.contextmanager
def thread_layout(tiles_x, tiles_y, order, filter):
    """the calling thread's layout for the duration of the block; the interlaced frame again afterwards"""
    from stm_amd import device_api as dev
    try:
        dev.set_layout(1, tiles_x, tiles_y, order, filter)
        yield
    finally:
        assert dev.lib().stm_set_layout(0, 0, 0, 0, 0) == 0
        dev.lib().stm_set_quilt_lds_limit(0)
        dev.lib().stm_set_agg_variant(0)


# ----------------------------------------------------------------------------- 1. the stage
# (views H x W), N, (tiles_x, tiles_y), (Ho x Wo), orders, staging limits (0 = the default)
STAGE_CASES = {
    "1x1_smallest": ((1, 1), 2, (2, 1), (1, 2), (0,), (0,)),
    "7x257_tile_straddles_a_block": ((7, 257), 6, (3, 2), (37, 771), (0, 3), (0,)),
    "40x64_integer_footprints": ((40, 64), 8, (4, 2), (40, 64), (0,), (0, 512)),
    "40x64_fractional_with_remainders": ((40, 64), 8, (4, 2), (45, 70), (0, 1, 2, 3), (0, 2048, 64)),
    "40x64_48_views": ((40, 64), 48, (8, 6), (96, 128), (3,), (0,)),
    "64x600_large_footprint": ((64, 600), 2, (2, 1), (4, 8), (0, 3), (0, 4096, 1024)),  # 1024: not one pixel's footprint fits -> per-pixel form
}


@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("case", list(STAGE_CASES), ids=list(STAGE_CASES))
def test_stage_both_flavours(gpu_ready, case, elem_sz):
    """stm_quilt_multiview and stm_d_quilt_multiview, both filters: bytes 0 .. 2 are the statement's (pixels of no tile 0); the device
    flavour leaves a fourth byte alone everywhere, the host flavour returns it 0; every staging limit gives the same bytes"""
    import torch
    from stm_amd import device_api as dev, host_api as api
    (H, W), N, (tx, ty), (Ho, Wo), orders, limits = STAGE_CASES[case]
    views = random_views(H * 31 + W + N, N, H, W, elem_sz)
    d_views = [torch.from_numpy(v).cuda() for v in views]
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    try:
        _arm(lib)
        for order in orders:
            for filter in (0, 1):
                want = quilt_ref(views, tx, ty, order, filter, Ho, Wo)
                for limit in (limits if filter == 1 else (0,)):
                    lib.stm_set_quilt_lds_limit(limit)
                    out = torch.full((Ho, Wo, elem_sz), FILL, dtype=torch.uint8, device="cuda")
                    dev.d_quilt_multiview(d_views, out, tx, ty, order, filter)
                    got = out.cpu().numpy()
                    assert np.array_equal(got[..., :3], want), (order, filter, limit, int((got[..., :3] != want).sum()))
                    assert (got[..., 3:] == FILL).all()
                    got = api.quilt_multiview(views, tx, ty, order, filter, Ho, Wo)
                    assert np.array_equal(got[..., :3], want), ("host", order, filter, limit)
                    assert (got[..., 3:] == 0).all()
        assert _clean(lib)
        for v, d in zip(views, d_views):
            assert np.array_equal(d.cpu().numpy(), v)  # read only
    finally:
        lib.stm_set_quilt_lds_limit(0)
        lib.stm_set_error_mode(0)


# ----------------------------------------------------------------------------- 2. the frame
H, W = 40, 64


def _check_maps(ch, dl, dr):
    assert np.array_equal(dl, ch["dl"]) and np.array_equal(dr, ch["dr"])  # the layout does not reach the maps


@pytest.mark.parametrize("stages", [3, 3 | LINEAR_WARP], ids=["0x3", "0x803"])
@pytest.mark.parametrize("elem_sz", [3, 4])
def test_frame_quilt_both_filters(gpu_ready, orc, elem_sz, stages):
    """stm_d_adcensus_stm under layout 1 at 45 x 70, 8 views as 4 x 2 tiles: both filters, two orders; the area filter with every
    staging limit (64: the per-pixel form); stm_set_agg_variant(200) -- every view written, then stm_k_quilt -- gives the same bytes"""
    from stm_amd import device_api as dev
    Ho, Wo, N = 45, 70, 8
    sbs, p = _frame(H, W), _params(N)
    ch = frame_chain(orc, sbs, p, stages & ~0xff)
    linear = bool(stages & LINEAR_WARP)
    lib = dev.lib()
    seen = set()
    for order in (0, 3):
        for filter in (0, 1):
            want = render_quilt_ref(orc, ch, N, 4, 2, order, filter, Ho, Wo, linear)
            with thread_layout(4, 2, order, filter):
                for limit in ((0, 2048, 64) if filter == 1 else (0,)):
                    lib.stm_set_quilt_lds_limit(limit)
                    dl, dr, out = _run(sbs, p, stages, Ho, Wo, elem_sz)
                    _check_maps(ch, dl, dr)
                    assert np.array_equal(out[..., :3], want), (order, filter, limit, int((out[..., :3] != want).sum()))
                    assert (out[..., 3:] == FILL).all()
                lib.stm_set_quilt_lds_limit(0)
                lib.stm_set_agg_variant(200)
                unfused = _run(sbs, p, stages, Ho, Wo, elem_sz)[2]
                lib.stm_set_agg_variant(0)
                assert np.array_equal(unfused, out), (order, filter)
            seen.add(out.tobytes())
    assert len(seen) == 4


@pytest.mark.parametrize("stages", [3, 3 | LINEAR_WARP], ids=["0x3", "0x803"])
def test_frame_quilt_with_manual_depth(gpu_ready, orc, stages):
    """depth mode 1 (0.6, 1.5): filter 1 averages the depth budget's views, filter 0 takes its sample rule at the tile's sampling
    position; 200 has no views to write and gives the same bytes"""
    from stm_amd import device_api as dev
    Ho, Wo, N = 45, 70, 8
    sbs, p = _frame(H, W), _params(N)
    ch = frame_chain(orc, sbs, p, 0)
    linear = bool(stages & LINEAR_WARP)
    lib = dev.lib()
    for filter in (0, 1):
        want = render_quilt_ref(orc, ch, N, 4, 2, 1, filter, Ho, Wo, linear, depth=(0.6, 1.5))
        with thread_layout(4, 2, 1, filter), thread_depth(1, 0.6, 1.5):
            for limit, variant in ((0, 0), (64, 0), (0, 200)):
                lib.stm_set_quilt_lds_limit(limit)
                lib.stm_set_agg_variant(variant)
                dl, dr, out = _run(sbs, p, stages, Ho, Wo)
                _check_maps(ch, dl, dr)
                assert np.array_equal(out, want), (filter, limit, variant, int((out != want).sum()))
        assert not np.array_equal(want, render_quilt_ref(orc, ch, N, 4, 2, 1, filter, Ho, Wo, linear))


def test_frame_quilt_with_automatic_depth(gpu_ready, orc):
    """depth mode 2: gain and conv come from the device-side fit of the maps the call returns; the caller's state is the statement's
    and is the same four floats with and without the layout"""
    import torch
    from stm_amd import device_api as dev
    Ho, Wo, N = 45, 70, 8
    sbs, p = _frame(H, W, 30), _params(N)
    lo, hi, mg, clip = AUTO
    lib = dev.lib()
    try:
        plain = torch.zeros(4, dtype=torch.float32, device="cuda")
        dev.set_depth_auto(lo, hi, mg, clip, 1.0, plain)
        with thread_depth(2):
            dl, dr, _ = _run(sbs, p, 3, Ho, Wo)
        want_st = depth_fit_ref(dl, dr, lo, hi, mg, clip, 1.0, np.zeros(4, f32))
        assert plain.cpu().numpy().tobytes() == want_st.tobytes()
        assert want_st[1] != 1 and want_st[1] != mg  # a fit that neither bound decides
        ch = _chain_of(orc, sbs, dl, dr)
        for filter in (0, 1):
            state = torch.zeros(4, dtype=torch.float32, device="cuda")
            dev.set_depth_auto(lo, hi, mg, clip, 1.0, state)
            with thread_layout(4, 2, 2, filter), thread_depth(2):
                dl2, dr2, out = _run(sbs, p, 3, Ho, Wo)
            assert np.array_equal(dl2, dl) and np.array_equal(dr2, dr)
            assert state.cpu().numpy().tobytes() == want_st.tobytes(), filter
            want = render_quilt_ref(orc, ch, N, 4, 2, 2, filter, Ho, Wo, False, depth=(want_st[1], want_st[2]))
            assert np.array_equal(out, want), (filter, int((out != want).sum()))
    finally:
        lib.stm_set_depth(0, 0.0, 0.0)
        lib.stm_set_depth_auto(-1.0, 1.0, 1.0, 20, 1.0, None)  # drop the pointer to this test's tensors


def test_retargeted_stereo_pair(gpu_ready, orc):
    """num_views 2 as 2 x 1 tiles, order 2 (the left camera first), at 40 x 150: tiles 75 wide from views 64 wide, so x is
    up-scaled.  Without a depth budget the pair is the two images; with gain 0.5 both are warps."""
    Ho, Wo, N = 40, 150, 2
    sbs, p = _frame(H, W), _params(N)
    ch = frame_chain(orc, sbs, p, 0)
    for filter in (0, 1):
        for depth in (None, (0.5, -1.0)):
            want = render_quilt_ref(orc, ch, N, 2, 1, 2, filter, Ho, Wo, False, depth=depth)
            with thread_layout(2, 1, 2, filter), thread_depth(0 if depth is None else 1, *(depth or (1.0, 0.0))):
                dl, dr, out = _run(sbs, p, 3, Ho, Wo)
            _check_maps(ch, dl, dr)
            assert np.array_equal(out, want), (filter, depth, int((out != want).sum()))
    # layout 1, filter 1, tiles of the views' own size, no depth budget: the pair itself, the left image first
    with thread_layout(2, 1, 2, 1):
        out = _run(sbs, p, 3, H, 2 * W)[2]
    assert np.array_equal(out[:, :W], ch["L"][..., :3]) and np.array_equal(out[:, W:], ch["R"][..., :3])


def test_reduced_frame(gpu_ready, orc):
    """stm_d_adcensus_stm_2s with 0x1000: the quilt is rendered from the guided up-scaled maps the call returns"""
    import torch
    from stm_amd import device_api as dev
    h, w, scale, Ho, Wo, N = 20, 32, 0.5, 45, 70, 8
    sbs, p = _frame(H, W, 3), _params(N)
    dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros((Ho, Wo, 3), dtype=torch.uint8, device="cuda")
    with thread_layout(4, 2, 3, 1):
        dev.d_adcensus_stm_2s(torch.from_numpy(np.array(sbs)).cuda(), dl, dr, out, p, h, w, scale, 3 | 0x1000)
        torch.cuda.synchronize()
    dl, dr = dl.cpu().numpy(), dr.cpu().numpy()
    want = render_quilt_ref(orc, _chain_of(orc, sbs, dl, dr), N, 4, 2, 3, 1, Ho, Wo)
    assert np.array_equal(out.cpu().numpy(), want)


def test_nv12_frame(gpu_ready, orc):
    import torch
    from stm_amd import device_api as dev, synth
    from test_nv12_ref import nv12_to_bgr_ref
    N = 8
    sbs, p = _frame(H, W, 7), _params(N)
    y, uv = synth.bgr_to_nv12(sbs, 1)
    bgr = np.ascontiguousarray(nv12_to_bgr_ref(y, uv, 1))
    ch = frame_chain(orc, bgr, p, LINEAR_WARP)
    dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros((45, 70, 3), dtype=torch.uint8, device="cuda")
    with thread_layout(4, 2, 0, 1):
        dev.d_adcensus_stm_nv12(torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(np.array(uv)).cuda(), dl, dr, out, p,
                                3 | LINEAR_WARP, matrix=1)
        torch.cuda.synchronize()
    _check_maps(ch, dl.cpu().numpy(), dr.cpu().numpy())
    assert np.array_equal(out.cpu().numpy(), render_quilt_ref(orc, ch, N, 4, 2, 0, 1, 45, 70, True))


def test_host_flavour(gpu_ready, orc):
    """stm_adcensus_stm, which ends in the device flavour's render"""
    from stm_amd import host_api as api
    Ho, Wo, N = 45, 70, 8
    sbs, p = _frame(H, W), _params(N)
    ch = frame_chain(orc, sbs, p, 0)
    args = (p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    with thread_layout(4, 2, 3, 1):
        dl, dr, out = api.adcensus_stm(np.array(sbs), W, Ho, Wo, *args)
    _check_maps(ch, dl, dr)
    assert np.array_equal(out, render_quilt_ref(orc, ch, N, 4, 2, 3, 1, Ho, Wo))


def test_a_call_that_renders_nothing_ignores_the_layout(gpu_ready, orc):
    """stages 2 stops before the renderer: a tiling that does not fit the call is no error there, the maps are the chain's and the
    output frame is not written"""
    from stm_amd import device_api as dev
    sbs, p = _frame(H, W), _params(8)
    ch = frame_chain(orc, sbs, p, 0)
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    try:
        _arm(lib)
        with thread_layout(3, 3, 0, 1):
            dl, dr, out = _run(sbs, p, 2, 45, 70)
        assert _clean(lib)
        _check_maps(ch, dl, dr)
        assert (out == FILL).all()
    finally:
        lib.stm_set_error_mode(0)


# ----------------------------------------------------------------------------- 3. the frame stream
def test_stream_layout_is_the_frame_call(gpu_ready):
    """four frames (the third and fourth replay the captured graphs) equal the per-frame call; stm_stream_set_layout after the first
    submit returns -1; the thread's own layout neither reaches the stream nor is changed by it"""
    from stm_amd import device_api as dev, video
    Ho, Wo = 45, 70
    p = _params(8)
    frames = [_frame(H, W, 20 + k) for k in range(4)]
    lib = dev.lib()
    layout = (1, 4, 2, 3, 1)
    fs = video.FrameStream(H, W, p, Ho, Wo, stages=3 | LINEAR_WARP, layout=layout)
    lib.stm_set_error_mode(1)
    got = []
    try:
        assert lib.stm_set_layout(1, 2, 4, 0, 0) == 0  # the thread's own: another tiling of the same views
        assert fs.submit(frames[0]) == 0
        assert lib.stm_stream_set_layout(fs._h, 1, 2, 4, 0, 0) == -1 and b"first submit" in lib.stm_last_error()
        assert dev.get_layout() == (1, 2, 4, 0, 0)
        assert fs.submit(frames[1]) == 1
        got.append(fs.collect())
        assert fs.submit(frames[2]) == 2
        got.append(fs.collect())
        assert fs.submit(frames[3]) == 3
        got.append(fs.collect())
        got.append(fs.collect())
        assert dev.get_layout() == (1, 2, 4, 0, 0)
    finally:
        fs.close()
        lib.stm_set_error_mode(0)
        assert lib.stm_set_layout(0, 0, 0, 0, 0) == 0
    for k, (_, dl, dr, out) in enumerate(got):
        with thread_layout(*layout[1:]):
            want = _run(frames[k], p, 3 | LINEAR_WARP, Ho, Wo)
        assert np.array_equal(dl, want[0]) and np.array_equal(dr, want[1]) and np.array_equal(out, want[2]), k
    with thread_layout(2, 4, 0, 0):
        assert not np.array_equal(_run(frames[0], p, 3 | LINEAR_WARP, Ho, Wo)[2], got[0][3])


# ----------------------------------------------------------------------------- 4. errors
def test_frame_errors_launch_nothing_and_name_the_argument(gpu_ready):
    from stm_amd import device_api as dev
    sbs = _frame(H, W)
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    # (layout, lens, num_views, (Ho, Wo), the word)
    cases = [((4, 2, 0, 1), (1, 8.0, 1.0, 0.0), 8, (45, 70), b"lens"), ((4, 2, 0, 0), None, 6, (45, 70), b"num_views"),
             ((3, 2, 0, 1), None, 8, (45, 70), b"num_views"), ((8, 1, 0, 1), None, 8, (45, 7), b"num_cols_out"),
             ((1, 8, 0, 0), None, 8, (7, 70), b"num_rows_out")]
    try:
        for lo, lens, N, (Ho, Wo), word in cases:
            _arm(lib)
            with thread_layout(*lo):
                if lens:
                    assert lib.stm_set_lens(*lens) == 0
                try:
                    dl, dr, out = _run(sbs, _params(N), 3, Ho, Wo)
                finally:
                    lib.stm_set_lens(0, 0.0, 0.0, 0.0)
            err = lib.stm_last_error()
            assert b"d_adcensus_stm:" in err and word in err, (lo, err)
            assert (out == FILL).all() and (dl == FILL).all() and (dr == FILL).all(), lo
    finally:
        lib.stm_set_error_mode(0)


# ----------------------------------------------------------------------------- 5. the default
def test_layout_0_is_the_frame_of_a_fresh_thread(gpu_ready):
    """layout 0 set explicitly, after a quilt was rendered on this thread, gives the bytes a thread that never heard of layouts gets"""
    from stm_amd import device_api as dev
    sbs, p = _frame(H, W), _params(8)
    with thread_layout(4, 2, 3, 1):
        quilt = _run(sbs, p, 3, 45, 70)
    dev.set_layout(0, 4, 2, 3, 1)
    here = _run(sbs, p, 3, 45, 70)
    box = {}

    def fresh():
        now = (C.c_int * 5)()
        dev.lib().stm_get_layout(now)
        box["layout"] = tuple(now)
        box["out"] = _run(sbs, p, 3, 45, 70)
        dev.lib().stm_release_workspace()

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert box["layout"] == (0, 1, 1, 0, 0)
    for a, b in zip(here, box["out"]):
        assert np.array_equal(a, b)
    assert not np.array_equal(here[2], quilt[2])
