"""View antialiasing on the GPU (stm_view_prefilter / stm_d_view_prefilter, stm_set_antialias, stm_stream_set_antialias), bit for bit
against the numpy statement of the definition (test_antialias_ref): the stage on every path of the kernel, the frame calls against
the existing numpy renderer statements applied to the statement's filtered images and the frame's own maps, the frame stream with
its graphs.  Every test leaves the thread's antialiasing, layout, output format, lens geometry and depth budget at mode 0."""
import contextlib

import numpy as np
import pytest

from test_antialias_ref import delta_for_half_width, prefilter_vec
from test_depth_ref import depth_fit_ref, render_depth_ref
from test_gpu_depth import AUTO, FILL, PANEL, _chain_of, _frame, _params, _run, thread_depth
from test_gpu_lens import thread_lens
from test_gpu_nv12out import _run_nv12, thread_output
from test_gpu_overlay import thread_overlay
from test_gpu_quilt import thread_layout
from test_lens_ref import LINEAR_WARP, chain_views, render_lens_ref
from test_nv12out_ref import nv12_surface_ref
from test_overlay_ref import overlay_ref, random_overlay, subpixel_shift_ref
from test_quilt_ref import render_quilt_ref

pytestmark = pytest.mark.gpu

f32 = np.float32
N = 8
AA = (3.0, 6, 1.0)  # strength, max_radius, gate: the 16-level frames reach K = 3 with it
INF, NAN = float("inf"), float("nan")


@contextlib.contextmanager
def thread_antialias(strength, max_radius, gate):
    """the calling thread's antialiasing for the duration of the block; off again afterwards, whatever happens"""
    from stm_amd import device_api as dev
    try:
        dev.set_antialias(1, strength, max_radius, gate)
        yield
    finally:
        dev.set_antialias(0)
        assert dev.get_antialias() == (0, 0.0, 0, 0.0)


# ----------------------------------------------------------------------------- 1. the stage
def _check_stage(img, disp, args, offsets=(0, 1, 2, 3), what=None):
    """both flavours against the statement: bytes 0 .. 2 are the statement's; the device flavour leaves the bytes past them as they
    were, the host flavour returns them 0.  The map stays 4-byte aligned (a float pointer): the images take every byte offset."""
    import torch
    from stm_amd import device_api as dev, host_api as api
    want = prefilter_vec(img, disp, *args)
    rows, cols, E = img.shape
    d_disp = torch.from_numpy(disp).cuda()
    for off in offsets:
        flat_i = torch.empty(img.size + 4, dtype=torch.uint8, device="cuda")
        flat_o = torch.full((img.size + 4,), FILL, dtype=torch.uint8, device="cuda")
        d_img, d_out = flat_i[off:off + img.size], flat_o[off:off + img.size]
        d_img.copy_(torch.from_numpy(img.reshape(-1)))
        dev._use_current_stream()
        dev.lib().stm_d_view_prefilter(d_out.data_ptr(), d_img.data_ptr(), d_disp.data_ptr(), rows, cols, E, *args)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().reshape(img.shape)
        assert np.array_equal(got[..., :3], want), (what, img.shape, args, off, int((got[..., :3] != want).sum()))
        assert (got[..., 3:] == FILL).all(), (what, off)                                      # fourth bytes untouched
        assert (flat_o[:off].cpu().numpy() == FILL).all() and (flat_o[off + img.size:].cpu().numpy() == FILL).all()
        assert np.array_equal(d_img.cpu().numpy().reshape(img.shape), img)                    # read only
    got = api.view_prefilter(img, disp, *args)
    assert np.array_equal(got[..., :3], want), (what, "host", img.shape, args)
    assert (got[..., 3:] == 0).all()
    return want


def _runs_map(rng, rows, cols):
    """runs of constant depth of 1 .. 40 pixels -- on the screen plane, sub-pixel, up to clamped -- with NaN and +-inf sprinkled in,
    and inside some runs a ripple of +-0.6 so that a gate of 1 keeps a neighbour one step away and rejects one two steps away"""
    levels = np.array([0.0, 0.0, 0.3, -0.4, 1.75, -3.5, 7.0, 14.0, -21.0, 28.0, 56.0, -120.0, 300.0], f32)
    d = np.zeros((rows, cols), f32)
    for y in range(rows):
        x = 0
        while x < cols:
            n = int(rng.randint(1, 41))
            d[y, x:x + n] = levels[rng.randint(len(levels))]
            if rng.randint(3) == 0:
                d[y, x:x + n] += (rng.randint(-1, 2, size=d[y, x:x + n].shape) * f32(0.6)).astype(f32)
            x += n
    k = max(1, rows * cols // 40)
    for v in (NAN, INF, -INF):
        d[rng.randint(rows, size=k), rng.randint(cols, size=k)] = v
    return d


# 300: the segment boundary at 256 falls inside blurred runs; 3 with max_radius 16 clamps at both ends inside one halo
WIDTHS = [1, 2, 3, 17, 63, 64, 65, 130, 257, 300]


@pytest.mark.parametrize("max_radius", [1, 8, 16])
@pytest.mark.parametrize("elem_sz", [3, 4])
def test_stage_shapes_offsets_and_special_values(gpu_ready, elem_sz, max_radius):
    """rows 1 .. 5, every width, caller buffers at every byte offset, maps with NaN, +-inf and sub-pixel values"""
    rng = np.random.RandomState(100 * elem_sz + max_radius)
    blurred = 0
    for i, cols in enumerate(WIDTHS):
        rows = 1 + i % 5
        img = rng.randint(0, 256, (rows, cols, elem_sz)).astype(np.uint8)
        disp = _runs_map(rng, rows, cols)
        for args in ((N, 1.0, max_radius, 1.0, 1.0, 0.0), (5, 2.5, max_radius, 0.5, 0.75, -2.0)):
            want = _check_stage(img, disp, args, what=(rows, cols))
            blurred += int(not np.array_equal(want, img[..., :3]))
    assert blurred >= 14
    # width 3, every pixel at the full radius: each side's taps are all the clamped end pixels
    img = rng.randint(0, 256, (2, 3, elem_sz)).astype(np.uint8)
    _check_stage(img, np.full((2, 3), 500.0, f32), (N, 1.0, max_radius, 1.0, 1.0, 0.0), what="width 3 clamped")


def _row_for_divisor(T, cols, centre):
    """a row of deltas whose centre pixel divides by T (strength 1, N = 8, max_radius 16, gate 1, gain 1, conv 0)"""
    if T % 2 == 0:  # every tap used on both sides: T = 16 + 2 H
        return np.full(cols, delta_for_half_width((T - 16) // 2), f32)
    w = (T - 16) % 16                 # odd: the last, partial tap is used on the left only
    a = (T - 16 - w) // 16            # whole taps used, left and right together
    K = (a + 1) // 2 + 1
    d0 = delta_for_half_width(16 * (K - 1) + w)
    row = np.full(cols, d0, f32)
    row[centre + K] = d0 + f32(1000.0)
    if a % 2 == 1:                    # one whole tap fewer on the right
        row[centre + K - 1] = d0 + f32(1000.0)
    return row


@pytest.mark.parametrize("elem_sz", [3, 4])
def test_every_divisor_beside_0_and_255(gpu_ready, elem_sz):
    """every T the rule can produce -- the even ones 16 .. 528 and the odd ones 17 .. 511 (an odd T takes exactly one partial tap,
    which leaves at most 30 whole ones) -- at a pixel whose neighbourhood holds only the bytes 0 and 255"""
    targets = list(range(16, 529, 2)) + list(range(17, 512, 2))
    cols, centre = 35, 17
    disp = np.stack([_row_for_divisor(T, cols, centre) for T in targets])
    rng = np.random.RandomState(9 + elem_sz)
    img = (rng.randint(0, 2, (len(targets), cols, elem_sz)) * 255).astype(np.uint8)
    args = (N, 1.0, 16, 1.0, 1.0, 0.0)
    _, T = prefilter_vec(img, disp, *args, return_T=True)
    assert T[:, centre].tolist() == targets
    assert T.min() == 16 and T.max() == 528
    _check_stage(img, disp, args, offsets=(0, 1), what="divisors")


@pytest.mark.parametrize("elem_sz", [3, 4])
def test_pass_through_wave_beside_a_blurred_wave(gpu_ready, elem_sz):
    """192 columns: wave 0 and wave 2 are all H = 0 (stored straight through), wave 1 is blurred and its gate of 1 keeps the taps one
    ripple step away and rejects those two steps away; the taps of wave 1's end pixels come from the pass-through waves' pixels"""
    rng = np.random.RandomState(21)
    img = rng.randint(0, 256, (3, 192, elem_sz)).astype(np.uint8)
    disp = np.zeros((3, 192), f32)
    disp[:, 64:128] = f32(28.0) + (rng.randint(-1, 2, (3, 64)) * f32(0.6)).astype(f32)
    args = (N, 1.0, 8, 1.0, 1.0, 0.0)
    want, T = prefilter_vec(img, disp, *args, return_T=True)
    assert (T[:, :64] == 16).all() and (T[:, 128:] == 16).all() and (T[:, 64:128] > 16).any()
    full = 16 + 2 * 32
    assert (T[:, 66:126] < full).any() and (T[:, 66:126] == full).any()  # some taps rejected, some pixels with all of them
    _check_stage(img, disp, args, offsets=(0, 1), what="waves")
    assert np.array_equal(want[:, :64], img[:, :64, :3])


# ----------------------------------------------------------------------------- 2. the frame calls
SIZES = [(48, 96), (37, 70)]


def _filtered_chain(orc, sbs, dl, dr, gain=1.0, conv=0.0, aa=AA):
    """the renderer's planes from the frame's own maps, with the statement's filtered images in place of the images"""
    ch = dict(_chain_of(orc, sbs, dl, dr))
    L, R = ch["L"], ch["R"]
    ch["L"] = np.ascontiguousarray(prefilter_vec(L, dl, N, *aa, gain, conv))
    ch["R"] = np.ascontiguousarray(prefilter_vec(R, dr, N, *aa, gain, conv))
    assert not np.array_equal(ch["L"], L[..., :3]) and not np.array_equal(ch["R"], R[..., :3])
    return ch


def _mux_ref(orc, ch, angle, Ho, Wo, linear=False, elem_sz=3):
    """the reference's interlacer on the chain's views; its view assignment depends on the pixel size, so the views get elem_sz bytes"""
    views = [np.concatenate([np.asarray(v)[..., :3], np.zeros(v.shape[:2] + (elem_sz - 3,), np.uint8)], axis=2)
             for v in chain_views(orc, ch, N, linear)]
    return orc.mux_multiview(views, angle, Ho, Wo)[..., :3]


def _on_off(run):
    """run() with the setting off and on: the maps are identical, the frames are not"""
    off = run()
    with thread_antialias(*AA):
        on = run()
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert not np.array_equal(on[2], off[2])
    return on


@pytest.mark.parametrize("case", ["plain", "plain_4_byte_pixels", "0x800", "agg_variant_200"])
@pytest.mark.parametrize("size", SIZES, ids=["48x96", "37x70"])
def test_frame_default_interlacer(gpu_ready, orc, size, case):
    from stm_amd import device_api as dev
    (H, W), p = size, _params(N)
    sbs = _frame(H, W)
    elem_sz = 4 if case == "plain_4_byte_pixels" else 3
    stages = 3 | (LINEAR_WARP if case == "0x800" else 0)
    try:
        dev.lib().stm_set_agg_variant(200 if case == "agg_variant_200" else 0)
        dl, dr, out = _on_off(lambda: _run(sbs, p, stages, H + 4, W + 7, elem_sz))
    finally:
        dev.lib().stm_set_agg_variant(0)
    want = _mux_ref(orc, _filtered_chain(orc, sbs, dl, dr), p.angle, H + 4, W + 7, bool(stages & LINEAR_WARP), elem_sz)
    assert np.array_equal(out[..., :3], want), int((out[..., :3] != want).sum())
    assert (out[..., 3:] == FILL).all()


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=["48x96", "37x70"])
def test_frame_lens_modes(gpu_ready, orc, size, mode):
    (H, W), p = size, _params(N)
    sbs = _frame(H, W)
    lens = (mode,) + PANEL
    with thread_lens(*lens):
        dl, dr, out = _on_off(lambda: _run(sbs, p, 3, H + 4, W + 7))
    want = render_lens_ref(orc, _filtered_chain(orc, sbs, dl, dr), N, lens, False, H + 4, W + 7)
    assert np.array_equal(out, want), int((out != want).sum())


@pytest.mark.parametrize("size", SIZES, ids=["48x96", "37x70"])
def test_frame_depth_mode_1(gpu_ready, orc, size):
    """the prefilter takes the budget's gain and conv: the blur follows the displayed disparity, not the measured one"""
    (H, W), p = size, _params(N)
    sbs = _frame(H, W)
    gain, conv = 0.6, -1.5
    with thread_depth(1, gain, conv):
        dl, dr, out = _on_off(lambda: _run(sbs, p, 3, H + 4, W + 7))
    ch = _filtered_chain(orc, sbs, dl, dr, gain, conv)
    want = render_depth_ref(ch, N, None, False, H + 4, W + 7, gain, conv, p.angle)
    assert np.array_equal(out, want), int((out != want).sum())
    plain = _filtered_chain(orc, sbs, dl, dr)  # gain 1, conv 0 would have blurred otherwise
    assert not np.array_equal(plain["L"], ch["L"])


@pytest.mark.parametrize("quilt", [False, True], ids=["interlaced", "quilt"])
@pytest.mark.parametrize("size", SIZES, ids=["48x96", "37x70"])
def test_frame_depth_mode_2_reads_the_fitted_state(gpu_ready, orc, size, quilt):
    """the fit runs before the prefilter, which reads gain and conv on the device; the caller's state is the fit's alone"""
    import torch
    from stm_amd import device_api as dev
    (H, W), p = size, _params(N)
    sbs = _frame(H, W, 30)
    lo, hi, mg, clip = AUTO
    lib = dev.lib()
    Ho, Wo = (48, 96) if quilt else (H + 4, W + 7)
    try:
        states = []
        outs = []
        for on in (False, True):
            state = torch.zeros(4, dtype=torch.float32, device="cuda")
            dev.set_depth_auto(lo, hi, mg, clip, 1.0, state)
            with contextlib.ExitStack() as stack:
                stack.enter_context(thread_depth(2))
                if quilt:
                    stack.enter_context(thread_layout(4, 2, 3, 1))
                if on:
                    stack.enter_context(thread_antialias(*AA))
                outs.append(_run(sbs, p, 3, Ho, Wo))
            states.append(state.cpu().numpy())
        (dl0, dr0, out0), (dl, dr, out) = outs
        assert np.array_equal(dl, dl0) and np.array_equal(dr, dr0) and not np.array_equal(out, out0)
        st = depth_fit_ref(dl, dr, lo, hi, mg, clip, 1.0, np.zeros(4, f32))
        assert states[0].tobytes() == st.tobytes() and states[1].tobytes() == st.tobytes()
        assert st[1] != 1.0  # the fit decided something
        ch = _filtered_chain(orc, sbs, dl, dr, st[1], st[2])
        if quilt:
            want = render_quilt_ref(orc, ch, N, 4, 2, 3, 1, Ho, Wo, False, depth=(st[1], st[2]))
        else:
            want = render_depth_ref(ch, N, None, False, Ho, Wo, st[1], st[2], p.angle)
        assert np.array_equal(out, want), int((out != want).sum())
    finally:
        lib.stm_set_depth(0, 0.0, 0.0)
        lib.stm_set_depth_auto(-1.0, 1.0, 1.0, 20, 1.0, None)  # drop the pointer to this test's tensor


@pytest.mark.parametrize("filter", [0, 1])
@pytest.mark.parametrize("size", SIZES, ids=["48x96", "37x70"])
def test_frame_quilt_bgr_and_nv12(gpu_ready, orc, size, filter):
    """a 4 x 2 quilt of 48 x 96 (even tiles): the BGR quilt and its NV12 surface, both from the filtered pair; with the un-fused
    form of variant 200 the end views are the filtered images too"""
    from stm_amd import device_api as dev
    (H, W), p = size, _params(N)
    sbs = _frame(H, W)
    Ho, Wo, matrix = 48, 96, 1
    lib = dev.lib()
    with thread_layout(4, 2, 3, filter):
        dl, dr, out = _on_off(lambda: _run(sbs, p, 3, Ho, Wo))
        with thread_antialias(*AA):
            lib.stm_set_agg_variant(200)
            unfused = _run(sbs, p, 3, Ho, Wo)[2]
            lib.stm_set_agg_variant(0)
            with thread_output(matrix):
                dl2, dr2, surface = _run_nv12(sbs, p, 3, Ho, Wo)
                lib.stm_set_agg_variant(200)
                surface_unfused = _run_nv12(sbs, p, 3, Ho, Wo)[2]
                lib.stm_set_agg_variant(0)
    want = render_quilt_ref(orc, _filtered_chain(orc, sbs, dl, dr), N, 4, 2, 3, filter, Ho, Wo, False)
    assert np.array_equal(out, want), int((out != want).sum())
    assert np.array_equal(unfused, want)
    assert np.array_equal(dl2, dl) and np.array_equal(dr2, dr)
    assert np.array_equal(surface, nv12_surface_ref(want, matrix))
    assert np.array_equal(surface_unfused, surface)


@pytest.mark.parametrize("size", SIZES, ids=["48x96", "37x70"])
def test_frame_reduced_resolution(gpu_ready, orc, size):
    import torch
    from stm_amd import device_api as dev
    (H, W), p = size, _params(N)
    sbs = _frame(H, W, 3)
    h, w = H // 2, W // 2

    def run():
        dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        dr = torch.zeros_like(dl)
        out = torch.full((H + 4, W + 7, 3), FILL, dtype=torch.uint8, device="cuda")
        dev.d_adcensus_stm_2s(torch.from_numpy(np.array(sbs)).cuda(), dl, dr, out, p, h, w, 0.5, 3 | 0x1000)
        torch.cuda.synchronize()
        return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()
    dl, dr, out = _on_off(run)
    want = _mux_ref(orc, _filtered_chain(orc, sbs, dl, dr), p.angle, H + 4, W + 7)
    assert np.array_equal(out, want), int((out != want).sum())


def test_nv12_input_keeps_its_converted_images(gpu_ready, orc):
    """stm_d_adcensus_stm_nv12: d_img_l / d_img_r, the next frame's history, are the unfiltered conversion with the setting on"""
    import torch
    from stm_amd import device_api as dev, synth
    H, W = SIZES[0]
    sbs, p = _frame(H, W, 7), _params(N)
    y, uv = synth.bgr_to_nv12(sbs, 1)

    def run():
        dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        dr = torch.zeros_like(dl)
        out = torch.full((H, W, 3), FILL, dtype=torch.uint8, device="cuda")
        il = torch.full((H, W, 3), FILL, dtype=torch.uint8, device="cuda")
        ir = torch.full_like(il, FILL)
        dev.d_adcensus_stm_nv12(torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(np.array(uv)).cuda(), dl, dr, out, p, 3, matrix=1,
                                img_l=il, img_r=ir)
        torch.cuda.synchronize()
        return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy(), il.cpu().numpy(), ir.cpu().numpy()
    off = run()
    with thread_antialias(*AA):
        on = run()
    for k in (0, 1, 3, 4):
        assert np.array_equal(on[k], off[k]), k
    assert not np.array_equal(on[2], off[2])
    ch = dict(_chain_of(orc, sbs, on[0], on[1]))
    ch["L"] = np.ascontiguousarray(prefilter_vec(on[3], on[0], N, *AA))
    ch["R"] = np.ascontiguousarray(prefilter_vec(on[4], on[1], N, *AA))
    assert np.array_equal(on[2], _mux_ref(orc, ch, p.angle, H, W))


def test_temporal_second_frame_keeps_its_maps(gpu_ready, orc):
    """0x2000: the second frame is stabilised on the unfiltered side-by-side frames, so its maps are the same with the setting on"""
    import torch
    from stm_amd import device_api as dev
    H, W = SIZES[1]
    p = _params(N)
    a, b = _frame(H, W, 0), _frame(H, W, 1)
    d_a, d_b = torch.from_numpy(np.array(a)).cuda(), torch.from_numpy(np.array(b)).cuda()

    def run():
        dla, dra, _ = _run(a, p, 3)
        hist = [torch.from_numpy(x).cuda() for x in (dla, dra)]
        dl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        dr = torch.zeros_like(dl)
        out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        dev.d_adcensus_stm_t(d_b, dl, dr, out, p, 3 | 0x2000, d_a, hist[0], hist[1], 0.5, 765, 100.0)
        torch.cuda.synchronize()
        return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()
    dl, dr, out = _on_off(run)
    assert not np.array_equal(dl, _run(b, p, 3)[0])  # the wide gates did blend the maps
    assert np.array_equal(d_a.cpu().numpy(), a) and np.array_equal(d_b.cpu().numpy(), b)
    assert np.array_equal(out, _mux_ref(orc, _filtered_chain(orc, b, dl, dr), p.angle, H, W))


def test_overlay_is_composited_unblurred(gpu_ready, orc):
    import torch
    H, W = SIZES[0]
    sbs, p = _frame(H, W), _params(N)
    ov = random_overlay(11, 6, 20)
    d_ov = torch.from_numpy(ov).cuda()
    with thread_antialias(*AA):
        base = _run(sbs, p, 3)[2]
        with thread_overlay(d_ov, 5, 3, 2.5):
            out = _run(sbs, p, 3)[2]
    want = overlay_ref(base, ov, 5, 3, 2.5, subpixel_shift_ref(orc, H, W, N))
    assert not np.array_equal(want, base)
    assert np.array_equal(out, want)


def test_host_flavour_and_a_call_that_renders_nothing(gpu_ready, orc):
    from stm_amd import host_api as api
    H, W = SIZES[1]
    sbs, p = _frame(H, W), _params(N)
    args = (p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    dl, dr, out = _on_off(lambda: api.adcensus_stm(np.array(sbs), W, H, W, *args))
    assert np.array_equal(out, _mux_ref(orc, _filtered_chain(orc, sbs, dl, dr), p.angle, H, W))
    # stages 2 stops before the renderer: the setting is ignored and the frame is not written
    plain = _run(sbs, p, 2)
    with thread_antialias(*AA):
        got = _run(sbs, p, 2)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and (got[2] == FILL).all()


# ----------------------------------------------------------------------------- 3. the frame stream
def test_stream_of_four_frames_with_graphs_is_the_frame_call(gpu_ready):
    """four frames: both slots replay their captured graphs for their second frame; the stream's own setting neither comes from the
    calling thread's nor changes it, and can be set only before the first submit"""
    from stm_amd import device_api as dev, video
    H, W = SIZES[0]
    p = _params(N)
    frames = [_frame(H, W, 50 + k) for k in range(4)]
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    got = []
    fs = video.FrameStream(H, W, p, antialias=AA)
    try:
        with thread_antialias(0.5, 2, 0.25):
            for k, f in enumerate(frames):
                if k >= 2:
                    got.append(fs.collect())
                assert fs.submit(f) == k
                if k == 0:
                    assert lib.stm_stream_set_antialias(fs._h, 1, 1.0, 8, 1.0) == -1 and b"first submit" in lib.stm_last_error()
            got.append(fs.collect())
            got.append(fs.collect())
            assert dev.get_antialias() == (1, 0.5, 2, 0.25)
    finally:
        lib.stm_set_error_mode(0)
        fs.close()
    plain = _run(frames[0], p, 3)
    with thread_antialias(*AA):
        for k, f in enumerate(frames):
            dl, dr, out = _run(f, p, 3)
            assert got[k][0] == k and np.array_equal(got[k][1], dl) and np.array_equal(got[k][2], dr), k
            assert np.array_equal(got[k][3], out), k
    assert not np.array_equal(got[0][3], plain[2])
    # a stream without the option is untouched by the thread's setting
    fs = video.FrameStream(H, W, p)
    try:
        with thread_antialias(*AA):
            assert fs.submit(frames[0]) == 0
            assert np.array_equal(fs.collect()[3], plain[2])
    finally:
        fs.close()


BAD = [((-0.5, 8, 1.0), "strength"), ((8.5, 8, 1.0), "strength"), ((NAN, 8, 1.0), "strength"), ((1.0, 0, 1.0), "max_radius"),
       ((1.0, 17, 1.0), "max_radius"), ((1.0, 8, -0.25), "gate"), ((1.0, 8, NAN), "gate"), ((1.0, 8, INF), "gate")]


def test_stream_setter_rules(gpu_ready):
    """every argument rule of stm_stream_set_antialias; a refused call leaves the stream's setting as it was"""
    from stm_amd import device_api as dev, video
    H, W = SIZES[1]
    p = _params(N)
    f = _frame(H, W)
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    fs = video.FrameStream(H, W, p)
    try:
        fs.set_antialias(1, *AA)
        for args, word in BAD:
            with pytest.raises(ValueError, match=word):
                fs.set_antialias(1, *args)
        for mode in (-1, 2):
            with pytest.raises(ValueError, match="mode"):
                fs.set_antialias(mode, *AA)
        assert fs.submit(f) == 0
        out = fs.collect()[3]
    finally:
        lib.stm_set_error_mode(0)
        fs.close()
    with thread_antialias(*AA):
        assert np.array_equal(out, _run(f, p, 3)[2])  # the accepted setting survived the refusals
    fs = video.FrameStream(H, W, p, antialias=AA)
    try:
        fs.set_antialias(0, NAN, -1, NAN)  # mode 0 ignores the rest
        assert fs.submit(f) == 0
        assert np.array_equal(fs.collect()[3], _run(f, p, 3)[2])
    finally:
        fs.close()
    assert dev.get_antialias()[0] == 0


# ----------------------------------------------------------------------------- 4. the tools
def _tool(name):
    """a tool's module, loaded in this process: its main() takes the argument vector"""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_video_tool_antialias(gpu_ready, tmp_path):
    """tools/stm_video.py --antialias on a directory of BMP frames: the interlaced frames are the per-frame calls' with the setting"""
    import copy
    from stm_amd import bmp_io
    H, W = SIZES[1]
    p = copy.copy(_params(N))
    p.angle = 18.0  # the tool truncates the angle as the reference's driver does
    frames = [_frame(H, W, 60 + k) for k in range(2)]
    for k, f in enumerate(frames):
        bmp_io.write_bmp(str(tmp_path / ("f%03d.bmp" % k)), np.array(f))
    out = tmp_path / "o"
    args = ["stm_video", str(tmp_path), str(N), "18.43", str(W), str(H), str(p.num_disp), str(p.zero_disp), str(p.ad_coeff),
            str(p.census_coeff), str(p.ucd), str(p.lcd), str(p.usd), str(p.lsd), str(p.thresh_s), str(p.thresh_h), str(out), "--antialias"]
    assert _tool("stm_video").main(args + [str(v) for v in AA]) == 0
    for k, f in enumerate(frames):
        got = bmp_io.read_bmp(str(out / ("interlaced_%05d.bmp" % k)))
        with thread_antialias(*AA):
            assert np.array_equal(got, _run(f, p, 3)[2]), k
        assert not np.array_equal(got, _run(f, p, 3)[2]), k


def test_image_tool_antialias(gpu_ready, orc, tmp_path):
    """tools/stm_image.py --antialias: every view, the end views included, comes from the pair filtered by its final maps -- without
    the option the end views are the inputs, with it they are not, and the maps do not see the option"""
    from stm_amd import bmp_io
    H, W = SIZES[1]
    sbs, p = _frame(H, W, 61), _params(N)
    L, R = orc.demux_sbs(np.array(sbs), W)
    bmp_io.write_bmp(str(tmp_path / "l.bmp"), L)
    bmp_io.write_bmp(str(tmp_path / "r.bmp"), R)
    base = ["stm_image", str(tmp_path / "l.bmp"), str(tmp_path / "r.bmp"), str(p.ad_coeff), str(p.census_coeff), str(p.num_disp),
            str(p.zero_disp), str(p.ucd), str(p.lcd), str(p.usd), str(p.lsd), str(N), "18.43", str(W), str(H), str(p.thresh_s), str(p.thresh_h)]
    main = _tool("stm_image").main
    assert main(base + [str(tmp_path / "plain")]) == 0
    assert main(base + [str(tmp_path / "aa"), "--antialias"] + [str(v) for v in AA]) == 0

    def read(d, n):
        return bmp_io.read_bmp(str(tmp_path / d / (n + ".bmp")))
    assert np.array_equal(read("plain", "view_%d" % (N - 1)), L) and np.array_equal(read("plain", "view_0"), R)
    assert not np.array_equal(read("aa", "view_%d" % (N - 1)), L) and not np.array_equal(read("aa", "view_0"), R)
    assert np.array_equal(read("aa", "disp_l"), read("plain", "disp_l"))
    assert not np.array_equal(read("aa", "interlaced"), read("plain", "interlaced"))
