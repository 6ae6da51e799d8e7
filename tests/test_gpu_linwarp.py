"""Linear sampling of the views' warps on the GPU (stm_dibr_dbm_lin / stm_d_dibr_dbm_lin, frame bit 0x800,
stm_stream_set_stages), bit for bit against the numpy statement of the definition (test_linwarp_ref) on the oracle's maps."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden, rand_pair
from test_linwarp_ref import (EDGE_CASES, EDGE_IDS, HSLO, INTERP, LINEAR_WARP, SHAPES, SHIFTS, SUBPIXEL, dbm_ref, edge_dbm_inputs,
                              linwarp_frame, warp_case)

pytestmark = pytest.mark.gpu


def _run(sbs, p, stages, H, W, fill=0, out_rows=None, out_cols=None):
    import torch
    from stm_amd import device_api as dev
    d_sbs = torch.from_numpy(sbs).cuda()
    dl = torch.full((H, W), float(fill), dtype=torch.float32, device="cuda")
    dr = torch.full_like(dl, float(fill))
    out = torch.full((out_rows or H, out_cols or W, 3), fill, dtype=torch.uint8, device="cuda")
    dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _both_flavours(orc, L, R, dl, dr, ml, mr, shift, linear=True):
    """host_api.dibr_dbm[_lin] (mask blur gaussian(7, 10)) and device_api.d_dibr_dbm_lin / stm_d_dibr_dbm (gaussian(10, 15)) on one
    case, each against dbm_ref; inputs are read only, bytes past a pixel's third come out 0.  Returns the device flavour's image."""
    import torch
    from stm_amd import device_api as dev, host_api as api
    H, W, E = L.shape
    keep = [a.copy() for a in (L, R, dl, dr, ml, mr)]
    occl = np.zeros((H, W), np.uint8)
    got = (api.dibr_dbm_lin if linear else api.dibr_dbm)(L, R, dl, dr, occl, occl, ml, mr, shift)
    assert got.shape == (H, W, E)
    assert np.array_equal(got[..., :3], dbm_ref(orc, L, R, dl, dr, ml, mr, shift, linear, 7, 10.0)), ("host", shift)
    assert not got[..., 3:].any()
    t = [torch.from_numpy(a).cuda() for a in (L, R, dl, dr, ml, mr)]
    out = torch.full((H, W, E), 99, dtype=torch.uint8, device="cuda")
    if linear:
        dev.d_dibr_dbm_lin(out, *t, shift)
    else:
        dev._use_current_stream()
        dev.lib().stm_d_dibr_dbm(*[dev._p(x) for x in [out] + t[:4]], None, None, dev._p(t[4]), dev._p(t[5]), shift, H, W, E)
    torch.cuda.synchronize()
    got_d = out.cpu().numpy()
    assert np.array_equal(got_d[..., :3], dbm_ref(orc, L, R, dl, dr, ml, mr, shift, linear, 10, 15.0)), ("device", shift)
    assert not got_d[..., 3:].any()
    for a, b, x in zip(keep, (L, R, dl, dr, ml, mr), t):
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, x.cpu().numpy(), equal_nan=True)
    return got_d


# ----------------------------------------------------------------------------- 1. per stage
@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_dbm_lin_known_answers(gpu_ready, orc, case, elem_sz):
    args, want = edge_dbm_inputs(case, elem_sz)
    got = _both_flavours(orc, *args)
    assert np.array_equal(got[..., :3], want), case[0]


@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_dbm_lin_random_maps(gpu_ready, orc, shape, elem_sz):
    """fractional maps with NaN, +-inf, whole numbers and positions far outside the row; one row, one column, two 256-wide blocks;
    on the fractional shifts the result is not dibr_dbm's (what fails without the feature)"""
    H, W = shape
    L, R, dl, dr, ml, mr = warp_case(100 + H, H, W, elem_sz)
    for shift in SHIFTS:
        lin = _both_flavours(orc, L, R, dl, dr, ml, mr, shift)
        near = _both_flavours(orc, L, R, dl, dr, ml, mr, shift, linear=False)
        if W > 1 and shift in SHIFTS[2:]:
            assert not np.array_equal(lin, near), shift
        if W == 1:
            assert np.array_equal(lin, near)


def test_dbm_lin_argument_errors(gpu_ready):
    import ctypes as C
    from stm_amd import device_api as dev
    lib = dev.lib()
    img = np.full((2, 3, 3), 7, np.uint8)
    m = np.zeros((2, 3), np.float32)
    u8p, f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    pi, pm = img.ctypes.data_as(u8p), m.ctypes.data_as(f32p)
    lib.stm_set_error_mode(1)
    try:
        for rows, cols, e, word in ((2, 3, 2, b"elem_sz"), (0, 3, 3, b"num_rows"), (2, 0, 3, b"num_cols")):
            lib.stm_last_error()
            lib.stm_dibr_dbm_lin(pi, pi, pi, pm, pm, None, None, pm, pm, 0.5, rows, cols, e)
            err = lib.stm_last_error()
            assert err and word in err and b"dibr_dbm_lin" in err, err
    finally:
        lib.stm_set_error_mode(0)
    assert np.all(img == 7)


# ----------------------------------------------------------------------------- 2. the frame
def _params(D, zd, usd, lsd, N=8):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd, num_views=N)


def _frame_vs_chain(orc, sbs, p, H, W, extra=0, out_rows=None, out_cols=None, differs=True):
    dl, dr, out = _run(sbs, p, 3 | LINEAR_WARP | extra, H, W, out_rows=out_rows, out_cols=out_cols)
    dl0, dr0, out0 = _run(sbs, p, 3 | extra, H, W, out_rows=out_rows, out_cols=out_cols)  # the same frame without the bit
    wl, wr, mux, _ = linwarp_frame(orc, sbs, p, extra, out_rows=out_rows, out_cols=out_cols)
    assert np.array_equal(dl, wl) and np.array_equal(dr, wr)
    assert np.array_equal(dl, dl0) and np.array_equal(dr, dr0)  # the bit changes the renderer only
    assert np.array_equal(out, mux)
    assert (not np.array_equal(out, out0)) == differs
    return out


@pytest.mark.parametrize("extra", [0, SUBPIXEL, INTERP, SUBPIXEL | INTERP, HSLO], ids=["plain", "subpixel", "interp", "both", "hslo"])
def test_frame_linwarp_vs_oracle_chain(gpu_ready, orc, extra):
    from stm_amd import synth
    H, W, D, zd = 48, 100, 16, 8
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + 64)
    _frame_vs_chain(orc, sbs, _params(D, zd, 17, 8), H, W, extra)


def test_frame_linwarp_resized_output(gpu_ready, orc):
    """37 x 83 rendered at 50 x 121: every resize tap has a non-zero weight somewhere, Hout % N != 0"""
    from stm_amd import synth
    H, W, D, zd = 37, 83, 24, 12
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + 61)
    _frame_vs_chain(orc, sbs, _params(D, zd, 20, 10), H, W, out_rows=50, out_cols=121)


def test_frame_linwarp_unfused_render(gpu_ready, orc):
    """stm_set_agg_variant(200): every view written by stm_k_view_synth_all, then interlaced"""
    from stm_amd import device_api as dev, synth
    H, W, D, zd = 40, 77, 32, 16
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + 6)
    lib = dev.lib()
    lib.stm_set_agg_variant(200)
    try:
        unfused = _frame_vs_chain(orc, sbs, _params(D, zd, 34, 17), H, W)
    finally:
        lib.stm_set_agg_variant(0)
    assert np.array_equal(unfused, _run(sbs, _params(D, zd, 34, 17), 3 | LINEAR_WARP, H, W)[2])


@pytest.mark.parametrize("N", [2, 5])
def test_frame_linwarp_view_counts(gpu_ready, orc, N):
    """N = 2: no synthesised view, the frame is the one without the bit; N = 5: three of them"""
    from stm_amd import synth
    H, W, D, zd = 48, 100, 16, 8
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + 64)
    _frame_vs_chain(orc, sbs, _params(D, zd, 17, 8, N), H, W, differs=N > 2)


# ----------------------------------------------------------------------------- 3. real content
def test_bud_pair_linwarp_subpixel_full_frame(gpu_ready, orc):
    """The real-content bud pair (640 x 384, D = 32) through stages 3 | 0x800 | 0x200"""
    from stm_amd import bmp_io, device_api as dev
    g = load_golden("bud_c1_golden")
    D, zd, ad, ce, ucd, lcd, usd, lsd, ts, th, N, angle = [float(x) for x in g["params"]]
    L, R = bmp_io.read_bmp(os.path.join(GOLDEN, "bud_2.bmp")), bmp_io.read_bmp(os.path.join(GOLDEN, "bud_3.bmp"))
    H, W, _ = L.shape
    sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
    p = dev.FrameParams(num_disp=int(D), zero_disp=int(zd), num_views=int(N), angle=angle, ad_coeff=ad, census_coeff=ce,
                        ucd=ucd, lcd=lcd, usd=int(usd), lsd=int(lsd), thresh_s=int(ts), thresh_h=th)
    _frame_vs_chain(orc, sbs, p, H, W, SUBPIXEL)


# ----------------------------------------------------------------------------- 4. errors
@pytest.mark.parametrize("stages", [1, 2])
def test_linwarp_without_rendering_is_an_error(gpu_ready, stages):
    """1 | 0x800 and 2 | 0x800 render nothing: they fail through stm_last_error before anything runs, the caller's buffers keep
    their contents"""
    from stm_amd import device_api as dev, synth
    H, W, D, zd = 24, 40, 16, 8
    sbs, _ = synth.sbs_frame(H, W, D, zd)
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    try:
        lib.stm_last_error()  # clear
        dl, dr, out = _run(sbs, _params(D, zd, 17, 8), stages | LINEAR_WARP, H, W, fill=7)
        err = lib.stm_last_error()
    finally:
        lib.stm_set_error_mode(0)
    assert err and b"0x800" in err, err
    assert np.all(dl == 7) and np.all(dr == 7) and np.all(out == 7)


# ----------------------------------------------------------------------------- 5. the default path
def test_default_path_untouched_by_the_new_bit(gpu_ready, orc):
    """The same frame with 0x800, without it, with it again: without it the result is the oracle's adcensus_stm"""
    H, W, D, zd = 56, 120, 32, 16
    L, R = rand_pair(H, W, 41)
    sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
    p = _params(D, zd, 17, 8)
    want = orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                            p.thresh_s, p.thresh_h)
    wl, wr, mux, _ = linwarp_frame(orc, sbs, p)
    runs = [_run(sbs, p, st, H, W) for st in (3 | LINEAR_WARP, 3, 3 | LINEAR_WARP, 3)]
    for dl, dr, out in (runs[1], runs[3]):
        assert np.array_equal(dl, want["disp_l"]) and np.array_equal(dr, want["disp_r"])
        assert np.array_equal(out, want["interlaced"])
    for dl, dr, out in (runs[0], runs[2]):
        assert np.array_equal(dl, wl) and np.array_equal(dr, wr) and np.array_equal(out, mux)
    assert not np.array_equal(runs[0][2], runs[1][2])


# ----------------------------------------------------------------------------- 6. the frame stream
def test_frame_stream_with_linwarp(gpu_ready):
    """stm_stream_set_stages(3 | 0x800): every frame of the stream (eager, captured and replayed ones) equals the device frame
    call with the same stages; the setter refuses 0x100, and anything after the first submit"""
    from stm_amd import device_api as dev, synth, video
    H, W, D, zd = 40, 72, 8, 4
    p = _params(D, zd, 9, 4)
    frames = [synth.sbs_frame(H, W, D, zd, seed=synth.SEED + 500 + k)[0] for k in range(6)]
    lib = dev.lib()
    fs = video.FrameStream(H, W, p)
    lib.stm_set_error_mode(1)
    try:
        lib.stm_last_error()
        assert lib.stm_stream_set_stages(fs._h, 3 | LINEAR_WARP | HSLO) == -1
        assert b"stages" in lib.stm_last_error()
        assert lib.stm_stream_set_stages(fs._h, 2 | LINEAR_WARP) == -1
        assert lib.stm_stream_set_stages(fs._h, 3 | LINEAR_WARP | SUBPIXEL | INTERP) == 0
        assert lib.stm_stream_set_stages(fs._h, 3 | LINEAR_WARP) == 0
        got, pending = [], 0
        for f in frames:
            if pending == 2:
                got.append(fs.collect())
                pending -= 1
            assert fs.submit(f) >= 0
            pending += 1
        assert lib.stm_stream_set_stages(fs._h, 3) == -1  # after a submit
        assert b"first submit" in lib.stm_last_error()
        with pytest.raises(ValueError):
            fs.set_stages(3 | LINEAR_WARP)
        while pending:
            got.append(fs.collect())
            pending -= 1
    finally:
        lib.stm_set_error_mode(0)
        fs.close()
    assert [g[0] for g in got] == list(range(6))
    differs = False
    for k, f in enumerate(frames):
        dl, dr, out = _run(f, p, 3 | LINEAR_WARP, H, W)
        assert np.array_equal(got[k][1], dl) and np.array_equal(got[k][2], dr) and np.array_equal(got[k][3], out), k
        differs |= not np.array_equal(out, _run(f, p, 3, H, W)[2])
    assert differs
