"""Pixels wider than 3 bytes (elem_sz = 4, and 6) through every image-taking entry of the C ABI, on the GPU.

Every case asserts three things:
 1. parity with the oracle on the same padded arrays, bit for bit: bytes 0..2 of image outputs, every float, arm and class output
    (the bars of test_gpu_parity.py; tests/test_pixel_stride_ref.py checks the oracle's side);
 2. padding independence, HIP against HIP: two different paddings give identical outputs, and -- except for the interlacer,
    whose row period round(num_views / tan(angle) / elem_sz) depends on elem_sz (d_mux_multiview.cu:146) -- the outputs equal
    those of the 3-byte call;
 3. the padding bytes of outputs.  Host flavour: 0 in every image output, whatever an earlier call left in the workspace
    (the reference clears its staging images, d_dibr_bwarp.cu:136-137, d_dibr_fwarp.cu:139-140; d_tx_scale.cu:95 does not,
    and would hand back uninitialised memory: here the bytes are 0 like the oracle's).  Device flavour, outputs pre-filled with
    0xA5: stm_d_dibr_dbm clears them (d_dibr_bwarp.cu:53), and so does stm_d_dibr_dfm -- the reference copies its whole cleared
    staging image over d_img_out (d_dibr_fwarp.cu:51,84) -- while stm_d_mux_multiview, stm_d_demux_sbs and the frame's
    interlaced image leave them untouched: the reference's kernels write three bytes per pixel and nothing clears those buffers
    (d_mux_multiview.cu:76-82, d_demux_common.cu, d_io.cu).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import rand_pair
from test_interp_ref import interp_frame
from test_pixel_stride_ref import padded

pytestmark = pytest.mark.gpu

# H, W, D, zd, usd, lsd: the smallest shapes that still cross the 64 x 16 front tiles, the 256-wide row blocks of the rendering
# kernels and the 16-row strips / 4-column groups of the aggregation; the last is whole 64-wide tiles with W % 4 == 0, where 3-byte
# input takes the front kernel's dword path and 4-byte input must not
SHAPES = [(37, 53, 7, 3, 9, 4), (50, 131, 20, 9, 34, 17), (32, 128, 8, 4, 17, 8)]
FRAMES = [(70, 131, 20, 9, 34, 17), (32, 128, 8, 4, 17, 8)]
FILL = 0xA5


@pytest.fixture(scope="module")
def api(gpu_ready):
    from stm_amd import host_api
    return host_api


def dirty_workspace(api):
    """Leaves 255 in the first MiB of the calling thread's workspace: an output staging buffer carved there by the next call
    shows in its padding bytes whether the call cleared it."""
    api.tx_scale(np.full((512, 512, 4), 255, np.uint8), 1, 1)


def check_image(got, want, E):
    assert got.shape == want.shape and got.shape[2] == E
    assert np.array_equal(got[..., :3], want[..., :3])
    assert not got[..., 3:].any(), "padding bytes of a host-flavour image output must be 0"


def maps_for(H, W, seed):
    rng = np.random.RandomState(seed)
    dl = rng.randint(-9, 6, size=(H, W)).astype(np.float32) + rng.random_sample((H, W)).astype(np.float32) * 0.9
    dr = rng.randint(-9, 6, size=(H, W)).astype(np.float32) + rng.random_sample((H, W)).astype(np.float32) * 0.9
    return dl, dr


def stage_cases():
    return [(s, 4) for s in SHAPES] + [(SHAPES[0], 6)]


# ----------------------------------------------------------------------------- stages, host flavour
@pytest.mark.parametrize("shape,E", stage_cases())
def test_ci_adcensus(api, orc, shape, E):
    H, W, D, zd, usd, lsd = shape
    L, R = rand_pair(H, W, 11 + H)
    c3 = api.ci_adcensus(L, R, 10.0, 30.0, D, zd)
    for seed in (1, 2):
        l, r = padded(L, E, seed), padded(R, E, seed + 10)
        got = api.ci_adcensus(l, r, 10.0, 30.0, D, zd)
        want = orc.ci_adcensus(l, r, 10.0, 30.0, D, zd)
        for k in (0, 1):
            assert np.array_equal(got[k], want[k])
            assert np.array_equal(got[k], c3[k])


@pytest.mark.parametrize("variant", [0, 10000])
@pytest.mark.parametrize("shape,E", stage_cases())
def test_ca_cross(api, orc, stm, shape, E, variant):
    H, W, D, zd, usd, lsd = shape
    L, R = rand_pair(H, W, 23 + W)
    cost, _ = orc.ci_adcensus(L, R, 10.0, 30.0, D, zd)
    stm.lib().stm_set_agg_variant(variant)
    try:
        x3, a3 = api.ca_cross(L, cost, 6.0, 20.0, usd, lsd)
        for seed in (1, 2):
            l = padded(L, E, seed)
            x, a = api.ca_cross(l, cost, 6.0, 20.0, usd, lsd)
            wx, wa = orc.ca_cross(l, cost, 6.0, 20.0, usd, lsd)
            assert np.array_equal(x, wx) and np.array_equal(a, wa)
            assert np.array_equal(x, x3) and np.array_equal(a, a3)
    finally:
        stm.lib().stm_set_agg_variant(0)


@pytest.mark.parametrize("shape", SHAPES)
def test_dc_hslo(api, orc, shape):
    H, W, D, zd, usd, lsd = shape
    L, R = rand_pair(H, W, 8 + W)
    c, _ = orc.ci_adcensus(L, R, 10.0, 30.0, D, zd)
    h3 = api.dc_hslo(c, L, R, 15.0, 1.0, 3.0, zd)
    for seed in (1, 2):
        l, r = padded(L, 4, seed), padded(R, 4, seed + 10)
        got = api.dc_hslo(c, l, r, 15.0, 1.0, 3.0, zd)
        assert np.array_equal(got, orc.dc_hslo(c, l, r, 15.0, 1.0, 3.0, zd))
        assert np.array_equal(got, h3)


@pytest.mark.parametrize("shape", SHAPES)
def test_dibr_dbm_and_dfm(api, orc, shape):
    H, W = shape[:2]
    L, R = rand_pair(H, W, 77)
    dl, dr = maps_for(H, W, H)
    ol, orr = orc.dibr_occl(dl, dr)
    ol, orr = orc.filter_bleed_1(ol, 1), orc.filter_bleed_1(orr, 1)
    ml, mr = orc.dibr_occl_to_mask(ol, orr)
    for shift in (float(np.float32(1.0 - 3.0 / 7.0)), 0.8):
        b3 = api.dibr_dbm(L, R, dl, dr, ol, orr, ml, mr, shift)
        f3 = api.dibr_dfm(L, R, dl, dr, shift)
        for seed in (1, 2):
            l, r = padded(L, 4, seed), padded(R, 4, seed + 10)
            dirty_workspace(api)
            got = api.dibr_dbm(l, r, dl, dr, ol, orr, ml, mr, shift)     # host flavour: gaussian(7, 10)
            check_image(got, orc.dibr_dbm(l, r, dl, dr, ml, mr, shift, 7, 10.0), 4)
            assert np.array_equal(got[..., :3], b3)
            dirty_workspace(api)
            got = api.dibr_dfm(l, r, dl, dr, shift)
            check_image(got, orc.dibr_dfm(l, r, dl, dr, shift), 4)
            assert np.array_equal(got[..., :3], f3)


@pytest.mark.parametrize("shape,E", stage_cases())
def test_tx_scale_down_and_up(api, orc, shape, E):
    H, W = shape[:2]
    L, _ = rand_pair(H, W, 5 + W)
    for (h, w) in [(H // 2 + 1, W // 2 - 3), (2 * H - 1, W + W // 3), (H, W)]:
        s3 = api.tx_scale(L, h, w)
        for seed in (1, 2):
            l = padded(L, E, seed)
            dirty_workspace(api)
            got = api.tx_scale(l, h, w)
            check_image(got, orc.tx_scale_bilinear(l, h, w), E)
            assert np.array_equal(got[..., :3], s3)


@pytest.mark.parametrize("N,angle", [(8, 18.43), (5, 25.0)])
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_mux_multiview(api, orc, shape, N, angle):
    """Hout % N == 0 (the reference's kernel_2) and != 0 (its general kernel, d_mux_multiview.cu:184-192)."""
    H, W = shape[:2]
    assert round(orc.mux_y_interval(N, angle, 4)) != round(orc.mux_y_interval(N, angle, 3))
    base = [rand_pair(H, W, 40 + v)[v & 1] for v in range(N)]
    for (Ho, Wo) in [(H + N - H % N, W + 8), (H + N - H % N + 3, W - 5), (2 * N, 3 * W)]:
        variant = 2 if Ho % N == 0 else 1
        outs = []
        for seed in (1, 2):
            views = [padded(b, 4, 100 * seed + v) for v, b in enumerate(base)]
            dirty_workspace(api)
            got = api.mux_multiview(views, angle, Ho, Wo)
            check_image(got, orc.mux_multiview(views, angle, Ho, Wo, variant), 4)
            outs.append(got)
        assert np.array_equal(outs[0], outs[1])
        assert not np.array_equal(outs[0][..., :3], api.mux_multiview(base, angle, Ho, Wo))  # another row period


# ----------------------------------------------------------------------------- frames
def _params(shape):
    from stm_amd import device_api as dev
    H, W, D, zd, usd, lsd = shape
    return dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd)


def _device_frame(sbs, p, stages, H, W):
    """stm_d_adcensus_stm with every output pre-filled with 0xA5 bytes; returns (disp_l, disp_r, interlaced, fill value of a float)."""
    import torch
    from stm_amd import device_api as dev
    E = sbs.shape[2]
    d_sbs = torch.from_numpy(sbs).cuda()
    raw = [torch.full((H * W * 4,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    dl, dr = [t.view(torch.float32).view(H, W) for t in raw]
    out = torch.full((H, W, E), FILL, dtype=torch.uint8, device="cuda")
    dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _oracle_frame(orc, sbs, p, stages, H, W):
    if stages & 0x400:
        wl, wr, mux, _ = interp_frame(orc, sbs, p, stages & 0xff, True)
        return wl, wr, mux
    f = orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd,
                         p.usd, p.lsd, p.thresh_s, p.thresh_h, stop_after_wta=(stages & 0xff) == 1, hslo=bool(stages & 0x100))
    if (stages & 0xff) == 1:
        return f["wta_l"], f["wta_r"], None
    return f["disp_l"], f["disp_r"], f["interlaced"]


@pytest.mark.parametrize("stages", [1, 2, 3, 3 | 0x100, 3 | 0x400], ids=["1", "2", "3", "3_hslo", "3_interp"])
@pytest.mark.parametrize("shape", FRAMES)
def test_device_frame(gpu_ready, orc, shape, stages):
    from stm_amd import synth
    H, W, D, zd = shape[:4]
    p = _params(shape)
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + W)
    a, b = padded(sbs, 4, 1), padded(sbs, 4, 2)
    ga, gb, g3 = _device_frame(a, p, stages, H, W), _device_frame(b, p, stages, H, W), _device_frame(sbs, p, stages, H, W)
    wl, wr, mux = _oracle_frame(orc, a, p, stages, H, W)
    assert np.array_equal(ga[0], wl) and np.array_equal(ga[1], wr)
    for k in (0, 1):
        assert np.array_equal(ga[k], gb[k]) and np.array_equal(ga[k], g3[k])
    assert np.array_equal(ga[2], gb[2])
    if (stages & 0xff) == 3:
        assert np.array_equal(ga[2][..., :3], mux[..., :3])
        assert (ga[2][..., 3] == FILL).all()  # three bytes per pixel are written, the fourth is the caller's
    else:
        assert (ga[2] == FILL).all()


@pytest.mark.parametrize("shape", FRAMES)
def test_host_frame(api, orc, shape):
    from stm_amd import synth
    H, W, D, zd = shape[:4]
    p = _params(shape)
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + H)
    args = (p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    g3 = api.adcensus_stm(sbs, W, H, W, *args)
    outs = []
    for seed in (1, 2):
        s = padded(sbs, 4, seed)
        got = api.adcensus_stm(s, W, H, W, *args)
        want = orc.adcensus_stm(s, H, W, *args)
        assert np.array_equal(got[0], want["disp_l"]) and np.array_equal(got[1], want["disp_r"])
        assert np.array_equal(got[0], g3[0]) and np.array_equal(got[1], g3[1])
        check_image(got[2], want["interlaced"], 4)
        outs.append(got[2])
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("shape,h,w", [(FRAMES[0], 40, 70), (FRAMES[1], 16, 64)])
def test_reduced_resolution_frame(api, orc, shape, h, w):
    from stm_amd import synth
    H, W, D, zd, usd, lsd = shape
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + 2 * H)
    scale = float(w) / float(W)
    D2, zd2 = max(D // 2, 2), zd // 2
    args = (8, 18.43, D2, zd2, 10.0, 30.0, 6.0, 20.0, 9, 4, 10, 0.2)
    g3 = api.adcensus_stm_2(sbs, W, H, W, h, w, scale, *args)
    outs = []
    for seed in (1, 2):
        s = padded(sbs, 4, seed)
        got = api.adcensus_stm_2(s, W, H, W, h, w, scale, *args)
        want = orc.adcensus_stm_2(s, H, W, h, w, scale, *args)
        assert np.array_equal(got[0], want["disp_l"]) and np.array_equal(got[1], want["disp_r"])
        assert np.array_equal(got[0], g3[0]) and np.array_equal(got[1], g3[1])
        check_image(got[2], want["interlaced"], 4)
        outs.append(got[2])
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("spare", [0, 1], ids=["Wsbs_2W", "Wsbs_2W_plus_1"])
@pytest.mark.parametrize("shape", FRAMES)
def test_d_demux_sbs(gpu_ready, stm, orc, shape, spare):
    import torch
    from stm_amd import synth
    H, W, D, zd = shape[:4]
    sbs, _ = synth.sbs_frame(H, W, D, zd)
    if spare:
        sbs = np.ascontiguousarray(np.concatenate([sbs, np.full((H, 1, 3), 200, np.uint8)], axis=1))
    l3, r3 = orc.demux_sbs(sbs, W)
    outs = []
    for seed in (1, 2):
        s = padded(sbs, 4, seed)
        d_s = torch.from_numpy(s).cuda()
        dL = torch.full((H, W, 4), FILL, dtype=torch.uint8, device="cuda")
        dR = torch.full_like(dL, FILL)
        P = lambda t: C.c_void_p(t.data_ptr())
        stm.lib().stm_d_demux_sbs(P(dL), P(dR), P(d_s), H, 2 * W + spare, W, 4)
        torch.cuda.synchronize()
        gl, gr = dL.cpu().numpy(), dR.cpu().numpy()
        wl, wr = orc.demux_sbs(s, W)
        assert np.array_equal(gl[..., :3], wl[..., :3]) and np.array_equal(gr[..., :3], wr[..., :3])
        assert np.array_equal(gl[..., :3], l3) and np.array_equal(gr[..., :3], r3)
        assert (gl[..., 3] == FILL).all() and (gr[..., 3] == FILL).all()  # d_demux_common.cu: three bytes per pixel are copied
        outs.append((gl, gr))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ----------------------------------------------------------------------------- device flavour: padding bytes of image outputs
def test_device_flavour_padding_bytes(gpu_ready, stm, orc):
    """stm_d_dibr_dbm and stm_d_dibr_dfm clear the caller's image (d_dibr_bwarp.cu:53; d_dibr_fwarp.cu:51,84),
    stm_d_mux_multiview writes three bytes per pixel and leaves the rest (d_mux_multiview.cu:76-82)."""
    import torch
    lib = stm.lib()
    H, W, N = 37, 53, 8
    L, R = rand_pair(H, W, 77)
    l, r = padded(L, 4, 1), padded(R, 4, 2)
    dl, dr = maps_for(H, W, 3)
    ol, orr = orc.dibr_occl(dl, dr)
    ml, mr = orc.dibr_occl_to_mask(orc.filter_bleed_1(ol, 1), orc.filter_bleed_1(orr, 1))
    P = lambda t: C.c_void_p(t.data_ptr())
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tl, tr, tdl, tdr, tol, tor, tml, tmr = T(l), T(r), T(dl), T(dr), T(ol), T(orr), T(ml), T(mr)
    out = torch.full((H, W, 4), FILL, dtype=torch.uint8, device="cuda")
    lib.stm_d_dibr_dbm(P(out), P(tl), P(tr), P(tdl), P(tdr), P(tol), P(tor), P(tml), P(tmr), C.c_float(0.4), H, W, 4)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), orc.dibr_dbm(l, r, dl, dr, ml, mr, 0.4, 10, 15.0))  # padding 0 included
    out.fill_(FILL)
    lib.stm_d_dibr_dfm(P(out), P(tl), P(tr), P(tdl), P(tdr), C.c_float(0.4), H, W, 4)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), orc.dibr_dfm(l, r, dl, dr, 0.4))
    views = [padded(rand_pair(H, W, 40 + v)[0], 4, v) for v in range(N)]
    tv = [T(v) for v in views]
    tab = torch.tensor([t.data_ptr() for t in tv], dtype=torch.int64).cuda()
    for (Ho, Wo) in [(40, 61), (43, 50)]:
        out = torch.full((Ho, Wo, 4), FILL, dtype=torch.uint8, device="cuda")
        lib.stm_d_mux_multiview(P(tab), P(out), N, C.c_float(18.43), H, W, Ho, Wo, 4)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[..., :3], orc.mux_multiview(views, 18.43, Ho, Wo, 2)[..., :3])  # the device flavour: always kernel_2
        assert (got[..., 3] == FILL).all()
