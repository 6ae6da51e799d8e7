"""Guided disparity up-sampling on the GPU (stm_disp_upsample / stm_d_disp_upsample, the reduced-resolution frame with a `stages`
word stm_adcensus_stm_2s / stm_d_adcensus_stm_2s and its bit 0x1000), bit for bit against the numpy statement of the definition
(test_upsample_ref) on the oracle's maps."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from test_upsample_ref import (FRAMES, GUIDED_UP, HSLO, INTERP, LINEAR_WARP, SHAPE_IDS, SHAPES, SIGMA, STRONG_REDUCTIONS, SUBPIXEL,
                               lone_colour_case, step_case, upsample_case, upsample_frame, upsample_ref)

pytestmark = pytest.mark.gpu

_REF = {}


def _case(orc, shape, elem_sz):
    """One random case per shape and pixel size with its reference, computed once and shared read-only"""
    key = (shape, elem_sz)
    if key not in _REF:
        (H, W), (h, w) = shape
        dlow, ilow, img = upsample_case(H * 7 + w + elem_sz, H, W, h, w, elem_sz)
        want, sw = upsample_ref(orc, dlow, ilow, img, 2.0, SIGMA, return_sw=True)
        for a in (dlow, ilow, img, want, sw):
            a.setflags(write=False)
        _REF[key] = (dlow, ilow, img, want, sw)
    return _REF[key]


def _both_flavours(dlow, ilow, img, up, sigma, want):
    """host_api.disp_upsample and device_api.d_disp_upsample against `want`; inputs are read only"""
    import torch
    from stm_amd import device_api as dev, host_api as api
    keep = [a.copy() for a in (dlow, ilow, img)]
    got = api.disp_upsample(dlow, ilow, img, up, sigma)
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True), "host"
    t = [torch.from_numpy(np.array(a)).cuda() for a in (dlow, ilow, img)]
    out = torch.full(img.shape[:2], 99.0, dtype=torch.float32, device="cuda")
    dev.d_disp_upsample(out, *t, up, sigma)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want, equal_nan=True), "device"
    for a, b, x in zip(keep, (dlow, ilow, img), t):
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, x.cpu().numpy(), equal_nan=True)


# ----------------------------------------------------------------------------- 1. per stage
@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_upsample_random_cases(gpu_ready, orc, shape, elem_sz):
    """images in flat patches (pixels with and without a tap of their colour), maps with NaN, +-inf and large values"""
    dlow, ilow, img, want, sw = _case(orc, shape, elem_sz)
    (H, W), _ = shape
    if H * W >= 60:
        assert (sw == 0).any() and (sw > 0).any()  # the fallback and the weighted mean both occur
        assert np.isnan(want).any() and np.isfinite(want).any()
    _both_flavours(dlow, ilow, img, 2.0, SIGMA, want)


def test_upsample_takes_both_branches_somewhere(orc):
    sws = [_case(orc, s, 3)[4] for s in SHAPES]
    assert any((sw == 0).any() for sw in sws) and any((sw > 0).any() for sw in sws)


@pytest.mark.parametrize("shape", STRONG_REDUCTIONS, ids=["%dx%d_from_%dx%d" % (s[0] + s[1]) for s in STRONG_REDUCTIONS])
def test_upsample_strong_reductions(gpu_ready, orc, shape):
    """reductions at which a block's taps no longer fit its staging buffer at the full tile size: the launcher's smaller tiles"""
    (H, W), (h, w) = shape
    dlow, ilow, img = upsample_case(H + w, H, W, h, w)
    for up, sigma in ((0.25, SIGMA), (1.0, 40.0)):
        _both_flavours(dlow, ilow, img, up, sigma, upsample_ref(orc, dlow, ilow, img, up, sigma))


@pytest.mark.parametrize("elem_sz", [3, 4])
def test_upsample_known_answers(gpu_ready, orc, elem_sz):
    dlow, ilow, img, up, want = step_case(elem_sz)
    assert np.array_equal(upsample_ref(orc, dlow, ilow, img, up, SIGMA), want)
    _both_flavours(dlow, ilow, img, up, SIGMA, want)
    dlow, ilow, img, up, (y, x) = lone_colour_case(elem_sz)
    want = upsample_ref(orc, dlow, ilow, img, up, SIGMA)
    assert want[y, x] == orc.tx_disp_scale(dlow, img.shape[0], img.shape[1], up)[y, x]
    _both_flavours(dlow, ilow, img, up, SIGMA, want)


def test_upsample_other_sigmas(gpu_ready, orc):
    """the table is per sigma_color: a narrow and a wide one after the frame's, then the frame's again"""
    dlow, ilow, img = upsample_case(77, 9, 37, 5, 19, nonfinite=False)
    for sigma in (SIGMA, 2.5, 60.0, SIGMA):
        _both_flavours(dlow, ilow, img, 2.0, sigma, upsample_ref(orc, dlow, ilow, img, 2.0, sigma))


def test_upsample_scattered_unaligned_buffers(gpu_ready, orc, stm):
    """every buffer carved from one arena at an odd / 4-byte-only aligned address; the margins stay untouched"""
    import torch
    from test_gpu_caller_buffers import Arena, P, read
    lib = stm.lib()
    lib.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for elem_sz in (3, 4):
        dlow, ilow, img, want, _ = _case(orc, SHAPES[3], elem_sz)
        (H, W), (h, w) = SHAPES[3]
        arena = Arena(True, nbytes=1 << 20)
        d_img, d_low, d_il = arena.put(img, 3), arena.put(dlow, 12), arena.put(ilow, 5)
        out = arena.carve(H * W * 4, 4)
        lib.stm_d_disp_upsample(P(out), P(d_low), P(d_il), P(d_img), H, W, h, w, elem_sz, 2.0, SIGMA)
        assert arena.intact()
        assert np.array_equal(read(out, np.float32, (H, W)), want, equal_nan=True)
        assert np.array_equal(read(d_img, np.uint8, img.shape), img) and np.array_equal(read(d_il, np.uint8, ilow.shape), ilow)
        assert np.array_equal(read(d_low, np.float32, dlow.shape), dlow, equal_nan=True)


def test_upsample_argument_errors(gpu_ready, stm):
    lib = stm.lib()
    u8p, f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    img = np.full((4, 6, 3), 7, np.uint8)
    low = np.full((2, 3, 3), 7, np.uint8)
    d = np.zeros((2, 3), np.float32)
    out = np.full((4, 6), 7, np.float32)
    po, pd, pl, pi = out.ctypes.data_as(f32p), d.ctypes.data_as(f32p), low.ctypes.data_as(u8p), img.ctypes.data_as(u8p)
    nan = float("nan")
    bad = [((4, 6, 2, 3, 2, 2.0, SIGMA), b"elem_sz"), ((0, 6, 2, 3, 3, 2.0, SIGMA), b"out_rows"), ((4, 0, 2, 3, 3, 2.0, SIGMA), b"out_cols"),
           ((4, 6, 0, 3, 3, 2.0, SIGMA), b"in_rows"), ((4, 6, 2, 0, 3, 2.0, SIGMA), b"in_cols"), ((4, 6, 2, 3, 3, 2.0, 0.0), b"sigma_color"),
           ((4, 6, 2, 3, 3, 2.0, nan), b"sigma_color"), ((4, 6, 2, 3, 3, 2.0, -1.0), b"sigma_color")]
    lib.stm_set_error_mode(1)
    try:
        for args, word in bad:
            lib.stm_last_error()
            lib.stm_disp_upsample(po, pd, pl, pi, *args)
            err = lib.stm_last_error()
            assert err and word in err and b"disp_upsample" in err and b"d_disp_upsample" not in err, err
            lib.stm_d_disp_upsample(None, None, None, None, *args)  # nothing is launched: the pointers are never used
            err = lib.stm_last_error()
            assert err and word in err and b"d_disp_upsample" in err, err
    finally:
        lib.stm_set_error_mode(0)
    assert np.all(out == 7)


# ----------------------------------------------------------------------------- 2. the frame
def _params(D, zd, usd, lsd, N=8):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd, num_views=N)


def _run2s(sbs, p, h, w, stages, fill=0, out_rows=None, out_cols=None, plain=False):
    """stm_d_adcensus_stm_2s (plain: stm_d_adcensus_stm_2) on buffers pre-filled with `fill`"""
    import torch
    from stm_amd import device_api as dev
    H, W = sbs.shape[0], sbs.shape[1] // 2
    d_sbs = torch.from_numpy(sbs).cuda()
    dl = torch.full((H, W), float(fill), dtype=torch.float32, device="cuda")
    dr = torch.full_like(dl, float(fill))
    out = torch.full((out_rows or H, out_cols or W, 3), fill, dtype=torch.uint8, device="cuda")
    scale = float(w) / float(W)
    if plain:
        dev._use_current_stream()
        dev.lib().stm_d_adcensus_stm_2(dev._p(d_sbs), dev._p(dl), dev._p(dr), dev._p(out), H, 2 * W, W, out.shape[0], out.shape[1], h, w,
                                       3, scale, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd,
                                       p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    else:
        dev.d_adcensus_stm_2s(d_sbs, dl, dr, out, p, h, w, scale, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _frame(dseed=0):
    from stm_amd import synth
    H, W, h, w, _ = FRAMES[0]
    return synth.sbs_frame(H, W, 32, 16, seed=synth.SEED + dseed)[0], _params(16, 8, 9, 4), h, w


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


STAGE_WORDS = [3 | GUIDED_UP, 3 | GUIDED_UP | LINEAR_WARP, 3 | GUIDED_UP | INTERP | SUBPIXEL, 3 | GUIDED_UP | HSLO, 3 | INTERP | LINEAR_WARP]


@pytest.mark.parametrize("stages", STAGE_WORDS, ids=["0x%x" % s for s in STAGE_WORDS])
def test_reduced_frame_with_stages_vs_oracle_chain(gpu_ready, orc, stages):
    """48 x 100 matched at 24 x 50, D = 16: maps and interlaced frame equal the composed chain; the new bit changes the maps (the
    left map of this frame is one value at half size, so it is the right one that moves)"""
    sbs, p, h, w = _frame()
    scale = float(w) / float(sbs.shape[1] // 2)
    got = _run2s(sbs, p, h, w, stages)
    want = upsample_frame(orc, sbs, p, h, w, scale, stages & ~0xff)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2])
    if stages & GUIDED_UP:
        base = _run2s(sbs, p, h, w, stages & ~GUIDED_UP)
        # (the maps, not the frame: with 0x400 | 0x200 they move by 0.02 at the most and the truncating fetch renders the same frame)
        assert not (np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]))


def test_reduced_frame_non_integer_ratio_resized_output(gpu_ready, orc):
    """37 x 83 matched at 19 x 41, rendered at 50 x 121; both maps change with the bit"""
    from stm_amd import synth
    H, W, h, w, dseed = FRAMES[1]
    sbs, _ = synth.sbs_frame(H, W, 32, 16, seed=synth.SEED + dseed)
    p = _params(16, 8, 9, 4)
    st = 3 | GUIDED_UP | LINEAR_WARP
    got = _run2s(sbs, p, h, w, st, out_rows=50, out_cols=121)
    want = upsample_frame(orc, sbs, p, h, w, float(w) / float(W), st & ~0xff, out_rows=50, out_cols=121)
    assert _same(got, want[:3])
    base = _run2s(sbs, p, h, w, 3 | LINEAR_WARP, out_rows=50, out_cols=121)
    assert not np.array_equal(got[0], base[0]) and not np.array_equal(got[1], base[1])


def test_reduced_frame_host_flavour(gpu_ready, orc):
    from stm_amd import host_api as api
    sbs, p, h, w = _frame()
    H, W = sbs.shape[0], sbs.shape[1] // 2
    scale = float(w) / float(W)
    st = 3 | GUIDED_UP | INTERP
    got = api.adcensus_stm_2s(sbs, W, H, W, h, w, scale, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd,
                              p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, stages=st)
    assert _same(got, upsample_frame(orc, sbs, p, h, w, scale, st & ~0xff)[:3])
    assert _same(got, _run2s(sbs, p, h, w, st))


def test_defaults_untouched_by_the_new_bit(gpu_ready, orc):
    """stm_d_adcensus_stm_2s(..., 3), stm_d_adcensus_stm_2 and the oracle's adcensus_stm_2 agree, before and after a 0x1000 call"""
    sbs, p, h, w = _frame()
    H, W = sbs.shape[0], sbs.shape[1] // 2
    o = orc.adcensus_stm_2(sbs, H, W, h, w, float(w) / float(W), p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff,
                           p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h)
    want = (o["disp_l"], o["disp_r"], o["interlaced"])
    assert _same(_run2s(sbs, p, h, w, 3), want) and _same(_run2s(sbs, p, h, w, 3, plain=True), want)
    guided = _run2s(sbs, p, h, w, 3 | GUIDED_UP)
    assert not _same(guided, want)
    assert _same(_run2s(sbs, p, h, w, 3), want) and _same(_run2s(sbs, p, h, w, 3, plain=True), want)


# ----------------------------------------------------------------------------- 3. errors
@pytest.mark.parametrize("stages,word", [(1 | GUIDED_UP, b"must be 3"), (2, b"must be 3"), (3 | SUBPIXEL | HSLO, b"0x200"), (3 | 0x2000, b"must be 3")],
                         ids=["low_byte_1", "low_byte_2", "0x300", "unknown_bit"])
def test_reduced_frame_stage_errors(gpu_ready, stages, word):
    """reported through stm_last_error with the call's name before anything runs: the buffers keep their fill value"""
    from stm_amd import device_api as dev, host_api as api
    sbs, p, h, w = _frame()
    H, W = sbs.shape[0], sbs.shape[1] // 2
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    try:
        lib.stm_last_error()
        dl, dr, out = _run2s(sbs, p, h, w, stages, fill=7)
        err = lib.stm_last_error()
        assert err and b"d_adcensus_stm_2s" in err and word in err, err
        assert np.all(dl == 7) and np.all(dr == 7) and np.all(out == 7)
        got = api.adcensus_stm_2s(sbs, W, H, W, h, w, 0.5, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff,
                                  p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, stages=stages)
        err = lib.stm_last_error()
        assert err and b"adcensus_stm_2s" in err and b"d_adcensus_stm_2s" not in err and word in err, err
        assert not any(a.any() for a in got)  # host_api's zero-initialised arrays, never written
    finally:
        lib.stm_set_error_mode(0)


def test_full_resolution_frame_rejects_the_bit(gpu_ready):
    import torch
    from stm_amd import device_api as dev, synth, video
    H, W, D, zd = 24, 40, 16, 8
    sbs, _ = synth.sbs_frame(H, W, D, zd)
    p = _params(D, zd, 17, 8)
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    fs = video.FrameStream(H, W, p)
    try:
        lib.stm_last_error()
        d_sbs = torch.from_numpy(sbs).cuda()
        dl = torch.full((H, W), 7.0, dtype=torch.float32, device="cuda")
        dr = torch.full_like(dl, 7.0)
        out = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda")
        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=3 | GUIDED_UP)
        torch.cuda.synchronize()
        err = lib.stm_last_error()
        assert err and b"0x1000" in err and b"d_adcensus_stm" in err, err
        assert bool((dl == 7).all()) and bool((dr == 7).all()) and bool((out == 7).all())
        assert lib.stm_stream_set_stages(fs._h, 3 | GUIDED_UP) == -1
        err = lib.stm_last_error()
        assert err and b"0x1000" in err and b"stream_set_stages" in err, err
        assert lib.stm_stream_set_stages(fs._h, 3 | LINEAR_WARP) == 0  # the stream is still usable
    finally:
        lib.stm_set_error_mode(0)
        fs.close()


# ----------------------------------------------------------------------------- 4. real content
def test_bud_pair_reduced_guided_linear(gpu_ready, orc):
    """The real-content bud pair (640 x 384) matched at 320 x 192, D = 16, through stages 3 | 0x1000 | 0x800"""
    from stm_amd import bmp_io, device_api as dev
    g = load_golden("bud_c1_golden")
    _, _, ad, ce, ucd, lcd, usd, lsd, ts, th, N, angle = [float(x) for x in g["params"]]
    L, R = bmp_io.read_bmp(os.path.join(GOLDEN, "bud_2.bmp")), bmp_io.read_bmp(os.path.join(GOLDEN, "bud_3.bmp"))
    H, W, _ = L.shape
    assert (H, W) == (384, 640)
    sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
    p = dev.FrameParams(num_disp=16, zero_disp=8, num_views=int(N), angle=angle, ad_coeff=ad, census_coeff=ce, ucd=ucd, lcd=lcd,
                        usd=int(usd) // 2, lsd=int(lsd) // 2, thresh_s=int(ts), thresh_h=th)
    st = 3 | GUIDED_UP | LINEAR_WARP
    got = _run2s(sbs, p, H // 2, W // 2, st)
    want = upsample_frame(orc, sbs, p, H // 2, W // 2, 0.5, st & ~0xff)
    assert _same(got, want[:3])
    assert not np.array_equal(got[0], _run2s(sbs, p, H // 2, W // 2, 3 | LINEAR_WARP)[0])
