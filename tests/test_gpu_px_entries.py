"""Every way into the frame at a size the pixel-major (PX) fast path takes: one small scenario -- 40 x 72, D = 64, usd 34 / lsd 17,
8 views -- at zero_disp 32 (stm_k_pq_hc<12, true>) and zero_disp 0 (stm_k_pq_hc<8, true>), through the host flavour, 4-byte pixels,
scattered caller buffers, NV12, packed input, the temporal frame, the reduced-resolution frame, the stage bits, the output
geometries and the frame stream.  PX changes the workspace carve, the vertical table's layout and the cross-arm kernel's table
output, which lie underneath all of them.

Each entry is compared with what the module of that feature compares it with (and through that module's own reference helpers),
element for element, and stm_agg_path is asked first whether the call is on the path the test is about."""
import ctypes as C

import numpy as np
import pytest

from conftest import rand_pair
from test_depth_ref import render_depth_ref
from test_gpu_caller_buffers import Arena, P, read
from test_gpu_depth import thread_depth
from test_gpu_px_layout import PQ_END_TO_END, _oracle
from test_gpu_quilt import thread_layout
from test_gpu_temporal import _recursion_t, _run as _run_fill
from test_gpu_upsample import _run2s
from test_interp_ref import interp_frame
from test_lens_ref import PANEL, frame_chain, render_lens_ref
from test_linwarp_ref import linwarp_frame
from test_nv12_ref import nv12_to_bgr_ref
from test_packing_ref import unpacked_sbs
from test_pixel_stride_ref import padded
from test_quilt_ref import render_quilt_ref
from test_temporal_ref import temporal_recursion
from test_upsample_ref import upsample_frame

pytestmark = pytest.mark.gpu

H, W, D, USD, LSD, N = 40, 72, 64, 34, 17, 8
HSLO, SUBPIXEL, INTERP, LINEAR_WARP, GUIDED_UP, T = 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000
FORMS = [(32, 12), (0, 8)]  # zero_disp -> waves per block of the first pass (hc_waves at D = 64, usd 34)
FORM_IDS = ["zd32_12waves", "zd0_8waves"]
form = pytest.mark.parametrize("zd, waves", FORMS, ids=FORM_IDS)


def _params(zd):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=zd, usd=USD, lsd=LSD, num_views=N)


_SBS = {}


def _frame(zd, seed_off=0):
    """the scenario's side-by-side frame; computed once, read only"""
    from stm_amd import synth
    if (zd, seed_off) not in _SBS:
        sbs = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + seed_off)[0]
        sbs.setflags(write=False)
        _SBS[(zd, seed_off)] = sbs
    return _SBS[(zd, seed_off)]


def _on_path(p, stages, waves, px=True, rows=H, cols=W):
    """stm_agg_path: the call is on PX with `waves` waves in stm_k_pq_hc -- or, px False, on the PQ layout"""
    from stm_amd import device_api as dev
    got = dev.agg_path(p.num_disp, p.zero_disp, rows, cols, p.usd, stages)
    assert got & dev.AGG_MATRIX_PIPE and bool(got & dev.AGG_PX) == px, "path 0x%x, stages 0x%x" % (got, stages)
    if px:
        assert dev.agg_path_waves(got) == waves and not got & dev.AGG_SPLIT, "path 0x%x, stages 0x%x" % (got, stages)
    return got


def _run(sbs, p, stages, Ho=None, Wo=None):
    """stm_d_adcensus_stm"""
    import torch
    from stm_amd import device_api as dev
    rows, cols = sbs.shape[0], sbs.shape[1] // 2
    dl = torch.zeros(rows, cols, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(Ho or rows, Wo or cols, 3, dtype=torch.uint8, device="cuda")
    dev.d_adcensus_stm(torch.from_numpy(np.array(sbs)).cuda(), dl, dr, out, p, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _same(got, want, what=""):
    assert len(got) >= 3 and len(want) >= 3
    for k, name in enumerate(("disp_l", "disp_r", "interlaced")):
        assert np.array_equal(got[k], want[k]), "%s %s" % (what, name)


def _oracle3(orc, sbs, p):
    f = _oracle(orc, np.array(sbs), p, sbs.shape[0], sbs.shape[1] // 2)
    return f["disp_l"], f["disp_r"], f["interlaced"]


# ----------------------------------------------------------------------------- host flavour, pixel sizes, caller buffers
@form
@pytest.mark.parametrize("elem_sz", [3, 4])
def test_host_flavour(gpu_ready, orc, zd, waves, elem_sz):
    """stm_adcensus_stm with 3- and 4-byte pixels against the oracle on the same bytes"""
    from stm_amd import host_api
    p = _params(zd)
    _on_path(p, 3, waves)
    sbs = np.array(_frame(zd)) if elem_sz == 3 else padded(_frame(zd), 4, 1)
    args = (p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    dl, dr, out = host_api.adcensus_stm(sbs, W, H, W, *args)
    want = orc.adcensus_stm(sbs, H, W, *args)
    assert np.array_equal(dl, want["disp_l"]) and np.array_equal(dr, want["disp_r"])
    assert out.shape == (H, W, elem_sz) and np.array_equal(out[..., :3], want["interlaced"][..., :3])
    assert not out[..., 3:].any()  # padding bytes of a host-flavour image output are 0


@form
def test_host_flavour_unaligned_buffers(gpu_ready, stm, orc, zd, waves):
    """stm_adcensus_stm on host buffers at odd addresses scattered over one allocation, guard bytes between them"""
    p = _params(zd)
    _on_path(p, 3, waves)
    sbs = _frame(zd)
    FILL, GAP = 0xA5, 4099
    sizes = [sbs.nbytes, H * W * 4, H * W * 4, H * W * 3]
    pool = np.full(sum(sizes) + 6 * GAP + 64, FILL, np.uint8)
    base = pool.ctypes.data
    offs, at = [], 0
    for n, mod in zip(sizes, (3, 4, 12, 9)):  # floats stay 4-byte aligned, bytes do not
        at += GAP
        at += (mod - (base + at)) % 16
        offs.append(at)
        at += n
    pool[offs[0]:offs[0] + sizes[0]] = sbs.reshape(-1)
    ptr = [C.cast(base + o, C.POINTER(C.c_float if k in (1, 2) else C.c_uint8)) for k, o in enumerate(offs)]
    stm.lib().stm_adcensus_stm(ptr[0], ptr[1], ptr[2], ptr[3], H, 2 * W, W, H, W, 3, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff,
                               p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    want = _oracle3(orc, sbs, p)
    got = [pool[offs[1]:offs[1] + sizes[1]].view(np.float32).reshape(H, W), pool[offs[2]:offs[2] + sizes[2]].view(np.float32).reshape(H, W),
           pool[offs[3]:offs[3] + sizes[3]].reshape(H, W, 3)]
    _same(got, want)
    assert np.array_equal(pool[offs[0]:offs[0] + sizes[0]], sbs.reshape(-1))
    keep = np.ones(pool.size, bool)
    for o, n in zip(offs, sizes):
        keep[o:o + n] = False
    assert (pool[keep] == FILL).all()


@form
@pytest.mark.parametrize("stages", [3, 3 | INTERP], ids=["0x3", "0x403"])
def test_scattered_device_buffers(gpu_ready, stm, orc, zd, waves, stages):
    """stm_d_adcensus_stm with the frame, both maps and the output at addresses 3, 4, 12 and 9 (mod 16) of one arena"""
    import torch
    p = _params(zd)
    _on_path(p, stages, waves)
    sbs = _frame(zd)
    want = interp_frame(orc, np.array(sbs), p, 3, True)[:3] if stages & INTERP else _oracle3(orc, sbs, p)
    lib = stm.lib()
    lib.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    arena = Arena(True, nbytes=1 << 20)
    src = arena.put(sbs, 3)
    dl, dr, out = arena.carve(H * W * 4, 4), arena.carve(H * W * 4, 12), arena.carve(H * W * 3, 9)
    lib.stm_d_adcensus_stm(P(src), P(dl), P(dr), P(out), H, 2 * W, W, H, W, 3, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff,
                           p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, stages)
    assert arena.intact()
    _same((read(dl, np.float32, (H, W)), read(dr, np.float32, (H, W)), read(out, np.uint8, (H, W, 3))), want)
    assert np.array_equal(read(src, np.uint8, sbs.shape), sbs)


# ----------------------------------------------------------------------------- NV12, packed input
@form
def test_nv12_frame(gpu_ready, orc, zd, waves):
    """stm_d_adcensus_stm_nv12 equals stm_d_adcensus_stm on the picture nv12_to_bgr_ref converts, and that frame equals the oracle"""
    import torch
    from stm_amd import device_api as dev, synth
    p = _params(zd)
    _on_path(p, 3, waves)
    y, uv = synth.bgr_to_nv12(np.array(_frame(zd)), 0)
    bgr = nv12_to_bgr_ref(y, uv, 0)
    assert bgr.shape == (H, 2 * W, 3)
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    il, ir = torch.zeros_like(out), torch.zeros_like(out)
    dev.d_adcensus_stm_nv12(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), dl, dr, out, p, 3, 0, il, ir)
    torch.cuda.synchronize()
    got = (dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy())
    want = _run(bgr, p, 3)
    _same(got, want, "nv12 against the BGR frame:")
    assert np.array_equal(il.cpu().numpy(), bgr[:, :W]) and np.array_equal(ir.cpu().numpy(), bgr[:, W:])
    _same(want, _oracle3(orc, bgr, p), "the BGR frame against the oracle:")


@form
@pytest.mark.parametrize("pk", [(1, 0, 1, 0), (2, 0, 0, 6)], ids=["half_width_catmull_rom", "top_and_bottom_gap6"])
def test_packed_input(gpu_ready, orc, zd, waves, pk):
    """the frame under stm_set_packing equals the frame on the pair the numpy statement unpacks (and that one the oracle)"""
    import torch
    from stm_amd import device_api as dev, synth
    p = _params(zd)
    _on_path(p, 3, waves)
    sbs = _frame(zd)
    packed = synth.pack_frame(np.array(sbs[:, :W]), np.array(sbs[:, W:]), pk[0], pk[1], pk[3], fill=0x33)
    plain = unpacked_sbs(packed, H, W, pk[:3], pk[3])
    assert plain.shape == (H, 2 * W, 3) and (pk[0] == 1) == (not np.array_equal(plain, sbs))
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    dev.set_packing(*pk)
    try:
        dev.d_adcensus_stm(torch.from_numpy(packed).cuda(), dl, dr, out, p, stages=3)
        torch.cuda.synchronize()
    finally:
        dev.set_packing(0, 0, 0, 0)
    want = _run(plain, p, 3)
    _same((dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()), want, "packed against unpacked:")
    _same(want, _oracle3(orc, plain, p), "the unpacked frame against the oracle:")


# ----------------------------------------------------------------------------- temporal frame, reduced-resolution frame
@form
def test_temporal_frame(gpu_ready, zd, waves):
    """stm_d_adcensus_stm_t at 2 | 0x2000 over three frames, each with the one before as its history: the maps of the frame without
    the bit followed by the numpy recursion"""
    p = _params(zd)
    _on_path(p, 2 | T, waves)
    _on_path(p, 2, waves)
    # the scenario's frame with a flat rectangle that moves 8 px per frame over both eyes (two columns apart, on the side of the
    # match range), under fresh noise of +-2 per channel -- test_temporal_ref.mixed_sequence's construction at this D
    rng, frames = np.random.RandomState(7), []
    for k in range(3):
        f = np.array(_frame(zd))
        for x0 in (6 + 8 * k, W + 6 + (-2 if zd else 2) + 8 * k):
            f[10:24, x0:x0 + 14] = (200, 60, 30)
        frames.append(np.clip(f.astype(np.int32) + rng.randint(-2, 3, size=f.shape), 0, 255).astype(np.uint8))
    plain = [_run_fill(f, p, 2)[:2] for f in frames]
    want = temporal_recursion(frames, plain)
    got = _recursion_t(frames, p, 2 | T)
    for k in range(3):
        assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]), k
        assert not got[k][2].any()  # stages 2 renders nothing
    assert any(not np.array_equal(want[k][v], plain[k][v]) for k in (1, 2) for v in (0, 1))  # the step did something


_BIG = {}


def _big_frame(zd):
    from stm_amd import synth
    if zd not in _BIG:
        _BIG[zd] = synth.sbs_frame(2 * H, 2 * W, 2 * D, 2 * zd, seed=synth.SEED + 5)[0]
        _BIG[zd].setflags(write=False)
    return _BIG[zd]


@form
def test_reduced_resolution_frame(gpu_ready, orc, zd, waves):
    """stm_d_adcensus_stm_2s, 80 x 144 matched at 40 x 72 with D = 64, against the oracle's adcensus_stm_2"""
    p = _params(zd)
    _on_path(p, 3, waves)
    sbs = np.array(_big_frame(zd))
    got = _run2s(sbs, p, H, W, 3)
    want = orc.adcensus_stm_2(sbs, 2 * H, 2 * W, H, W, 0.5, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd,
                              p.lsd, p.thresh_s, p.thresh_h)
    _same(got, (want["disp_l"], want["disp_r"], want["interlaced"]))


@form
def test_reduced_resolution_frame_guided(gpu_ready, orc, zd, waves):
    """... and with 0x1000 against the chain test_upsample_ref composes"""
    p = _params(zd)
    _on_path(p, 3 | GUIDED_UP, waves)
    sbs = np.array(_big_frame(zd))
    got = _run2s(sbs, p, H, W, 3 | GUIDED_UP)
    _same(got, upsample_frame(orc, sbs, p, H, W, 0.5, GUIDED_UP))


# ----------------------------------------------------------------------------- stage bits
def _stage_reference(orc, sbs, p, stages):
    sbs = np.array(sbs)
    if stages == 3 | INTERP:
        return interp_frame(orc, sbs, p, 3, True)[:3]
    if stages == 3 | LINEAR_WARP:
        return linwarp_frame(orc, sbs, p, 0, True)[:3]
    if stages == 3 | SUBPIXEL:
        return interp_frame(orc, sbs, p, 3, False, subpixel=True)[:3]
    assert stages == 3 | HSLO
    f = orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, D, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                         p.thresh_s, p.thresh_h, hslo=True)
    return f["disp_l"], f["disp_r"], f["interlaced"]


# PX and not PX alternating: 0x400 and 0x800 leave the aggregation alone, 0x200 and 0x100 read a volume after it
STAGE_WORDS = [(3 | INTERP, True), (3 | SUBPIXEL, False), (3 | LINEAR_WARP, True), (3 | HSLO, False)]


@form
def test_stage_bits_one_after_the_other_in_one_workspace(gpu_ready, stm, orc, zd, waves):
    """3 | 0x400 and 3 | 0x800 stay on PX, 3 | 0x200 and 3 | 0x100 leave it; each equals its module's reference.  Then the four back
    to back in one workspace, twice round: the window tables' and the volumes' layouts change from call to call, and every call
    still gives what it gives alone in a fresh workspace."""
    p = _params(zd)
    sbs = _frame(zd)
    lib = stm.lib()
    alone = {}
    for stages, px in STAGE_WORDS:
        _on_path(p, stages, waves, px)
        lib.stm_release_workspace()
        alone[stages] = _run(sbs, p, stages)
        _same(alone[stages], _stage_reference(orc, sbs, p, stages), "stages 0x%x alone:" % stages)
    lib.stm_release_workspace()
    for lap in (0, 1):
        for stages, _ in STAGE_WORDS:
            _same(_run(sbs, p, stages), alone[stages], "stages 0x%x, lap %d:" % (stages, lap))


# ----------------------------------------------------------------------------- output geometries
@form
def test_output_geometries(gpu_ready, orc, zd, waves):
    """a lens mode 2 frame, a manual depth budget and a 4 x 2 quilt, all rendered at 45 x 70 from the maps of the PX chain"""
    p = _params(zd)
    _on_path(p, 3, waves)
    sbs = _frame(zd)
    Ho, Wo = 45, 70
    ch = frame_chain(orc, np.array(sbs), p, 0)
    lens = (2,) + PANEL
    with thread_depth(0, lens=lens):
        dl, dr, out = _run(sbs, p, 3, Ho, Wo)
    _same((dl, dr, out), (ch["dl"], ch["dr"], render_lens_ref(orc, ch, N, lens, False, Ho, Wo)), "lens mode 2:")
    with thread_depth(1, 0.5, 2.0):
        dl, dr, out = _run(sbs, p, 3, Ho, Wo)
    _same((dl, dr, out), (ch["dl"], ch["dr"], render_depth_ref(ch, N, None, False, Ho, Wo, 0.5, 2.0, p.angle, 3)), "depth budget:")
    with thread_layout(4, 2, 0, 1):
        dl, dr, out = _run(sbs, p, 3, Ho, Wo)
    _same((dl, dr, out), (ch["dl"], ch["dr"], render_quilt_ref(orc, ch, N, 4, 2, 0, 1, Ho, Wo)), "quilt:")
    _same(_run(sbs, p, 3), _oracle3(orc, sbs, p), "defaults again:")


# ----------------------------------------------------------------------------- frame stream
@form
@pytest.mark.parametrize("variant", [0, PQ_END_TO_END], ids=["default", "pq_end_to_end"])
def test_frame_stream(gpu_ready, stm, orc, zd, waves, variant):
    """video.FrameStream over nine frames written into its zero-copy buffers (from its third frame on a slot replays its captured
    graph), with a larger per-stage call between submissions that regrows the thread's shared workspace: every frame equals the
    per-frame call, and frame 3 the oracle.  The variant is set before the stream is created and restored after it is closed."""
    from stm_amd import device_api as dev, host_api, video
    p = _params(zd)
    lib = stm.lib()
    frames = [_frame(zd, 100 + k) for k in range(9)]
    big_l, big_r = rand_pair(300, 500, 77)
    lib.stm_set_agg_variant(variant)
    try:
        got_path = dev.agg_path(D, zd, H, W, USD, 3)
        assert bool(got_path & dev.AGG_PX) == (variant == 0) and dev.agg_path_waves(got_path) == waves, hex(got_path)
        fs = video.FrameStream(H, W, p)
        try:
            got, pending = [], 0
            for k, f in enumerate(frames):
                if pending == 2:
                    got.append(fs.collect())
                    pending -= 1
                buf = fs.input_buffer()
                assert buf is not None and buf.shape == f.shape
                buf[...] = f
                assert fs.submit_inplace() == k
                pending += 1
                if k in (3, 6):
                    host_api.ci_adcensus(big_l, big_r, 10.0, 30.0, 24, 12)
            while pending:
                got.append(fs.collect())
                pending -= 1
        finally:
            fs.close()
        assert [g[0] for g in got] == list(range(9))
        for k, f in enumerate(frames):
            _same(got[k][1:], _run(f, p, 3), "frame %d against the per-frame call:" % k)
    finally:
        lib.stm_set_agg_variant(0)
    _same(got[3][1:], _oracle3(orc, frames[3], p), "frame 3 against the oracle:")
    assert b"outlier list" not in lib.stm_last_error()
