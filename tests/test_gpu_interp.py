"""Outlier interpolation on the GPU (stm_dr_interp / stm_d_dr_interp, frame bit 0x400, stm_stream_set_stages), bit for bit
against the numpy statement of the definition (test_interp_ref) applied to the oracle's maps: the step copies values, there is
nothing to tolerate."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden, rand_pair
from test_interp_ref import RANDOM_CASES, ROW_DISP, grey, interp_frame, interp_ref, interp_ref_fast, random_case

pytestmark = pytest.mark.gpu

INTERP, SUBPIXEL, HSLO = 0x400, 0x200, 0x100


def _run(sbs, p, stages, H, W, fill=0):
    import torch
    from stm_amd import device_api as dev
    d_sbs = torch.from_numpy(sbs).cuda()
    dl = torch.full((H, W), float(fill), dtype=torch.float32, device="cuda")
    dr = torch.full_like(dl, float(fill))
    out = torch.full((H, W, 3), fill, dtype=torch.uint8, device="cuda")
    dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _both_flavours(disp, outl, img, want, changes=True):
    """host_api.dr_interp and device_api.d_dr_interp on one case; `changes`: the expected result differs from the input"""
    import torch
    from stm_amd import device_api as dev, host_api as api
    assert (not np.array_equal(want, disp, equal_nan=True)) == changes
    disp0, outl0, img0 = disp.copy(), outl.copy(), img.copy()
    got = api.dr_interp(disp, outl, img)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(disp, disp0, equal_nan=True) and np.array_equal(outl, outl0) and np.array_equal(img, img0)
    d_disp, d_outl, d_img = torch.from_numpy(disp).cuda(), torch.from_numpy(outl).cuda(), torch.from_numpy(img).cuda()
    dev.d_dr_interp(d_disp, d_outl, d_img)
    torch.cuda.synchronize()
    assert np.array_equal(d_disp.cpu().numpy(), want, equal_nan=True)
    assert np.array_equal(d_outl.cpu().numpy(), outl0) and np.array_equal(d_img.cpu().numpy(), img0)  # read only


def _known_answers():
    cases = []
    cases.append((ROW_DISP.copy(), np.array([[0, 0, 2, 2, 2, 0, 0]], np.uint8), grey([[0] * 7]), [[3, 3, 3, 3, 3, -2, -2]]))
    mis = np.array([[0, 0, 1, 1, 7, 0, 0]], np.uint8)
    cases.append((ROW_DISP.copy(), mis, grey([[10, 10, 190, 200, 215, 200, 200]]), [[3, 3, -2, -2, -2, -2, -2]]))
    cases.append((ROW_DISP.copy(), mis, grey([[90, 90, 100, 100, 100, 110, 110]]), [[3, 3, -2, -2, -2, -2, -2]]))
    disp = np.arange(15, dtype=np.float32).reshape(3, 5)  # the knight's move: (0, 0) reaches (4, 2), (1, 0) reaches nothing
    outl = np.ones((3, 5), np.uint8)
    outl[2, 4] = 0
    want = interp_ref(disp, outl, grey(np.zeros((3, 5))))
    assert want[0, 0] == 14 and want[0, 1] == 1
    cases.append((disp, outl, grey(np.zeros((3, 5))), want.tolist()))
    nan = np.nan
    occ = np.array([[0, 2, 0]], np.uint8)
    cases.append((np.array([[5, 1, nan]], np.float32), occ, grey([[0, 0, 0]]), [[5, nan, nan]]))  # NaN first: it stays
    cases.append((np.array([[nan, 1, 5]], np.float32), occ, grey([[0, 0, 0]]), [[nan, 5, 5]]))  # NaN later: never enters
    return cases


@pytest.mark.parametrize("k", range(6))
def test_dr_interp_known_answers(gpu_ready, k):
    disp, outl, img, want = _known_answers()[k]
    want = np.array(want, np.float32)
    assert np.array_equal(interp_ref(disp, outl, img), want, equal_nan=True)
    _both_flavours(disp, outl, img, want)


@pytest.mark.parametrize("case", RANDOM_CASES, ids=["%dx%dx%d" % c[1:4] for c in RANDOM_CASES])
def test_dr_interp_random_maps(gpu_ready, case):
    """classes 0, 1, 2 and 7, NaN and fractions in the map, three grey levels (colour ties); H = 1, W = 1, elem_sz = 4, widths that
    are not a multiple of 64"""
    disp, outl, img = random_case(*case)
    _both_flavours(disp, outl, img, interp_ref(disp, outl, img))


def test_dr_interp_larger_random_map_spans_several_blocks(gpu_ready):
    disp, outl, img = random_case(21, 67, 203, 3, 0.3)  # 13601 pixels: several compaction blocks, walks across their borders
    want = interp_ref_fast(disp, outl, img)
    _both_flavours(disp, outl, img, want)


@pytest.mark.parametrize("which", ["all_outlier", "all_reliable"])
def test_dr_interp_nothing_to_do(gpu_ready, which):
    disp, outl, img = random_case(31, 19, 45)
    outl[...] = 0 if which == "all_reliable" else 1
    if which == "all_outlier":
        outl[::3] = 2
    _both_flavours(disp, outl, img, disp.copy(), changes=False)


def test_dr_interp_on_the_oracles_post_voting_maps(gpu_ready, orc):
    from stm_amd import device_api as dev, synth
    H, W, D, zd = 64, 120, 16, 8
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + 9)
    _, _, _, info = interp_frame(orc, sbs, dev.FrameParams(num_disp=D, zero_disp=zd, usd=17, lsd=8), 2, True)
    for side in "lr":
        disp, outl, img = info["voted_" + side], info["outl_" + side], info["img_" + side]
        assert set(np.unique(outl)) == {0, 1, 2}
        _both_flavours(disp, outl, img, interp_ref(disp, outl, img))


def test_dr_interp_argument_errors(gpu_ready):
    from stm_amd import device_api as dev
    import ctypes as C
    lib = dev.lib()
    disp = np.full((2, 3), 7, np.float32)
    outl = np.ones((2, 3), np.uint8)
    img = np.zeros((2, 3, 3), np.uint8)
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    lib.stm_set_error_mode(1)
    try:
        for rows, cols, e, word in ((2, 3, 2, b"elem_sz"), (0, 3, 3, b"num_rows"), (2, 0, 3, b"num_cols")):
            lib.stm_last_error()
            lib.stm_dr_interp(disp.ctypes.data_as(f32p), outl.ctypes.data_as(u8p), img.ctypes.data_as(u8p), rows, cols, e)
            err = lib.stm_last_error()
            assert err and word in err, err
    finally:
        lib.stm_set_error_mode(0)
    assert np.all(disp == 7)


# (name, H, W, D, zd, usd, lsd, aggregation variant, seed): the sizes and variants of test_gpu_subpixel.CASES, on seeds whose frames
# leave region voting something that the step can fill in both views
CASES = [
    ("ring_d16", 48, 100, 16, 8, 17, 8, 0, 64),
    ("pq_hs_d80", 32, 90, 80, 40, 34, 17, 0, 5),
    ("quads_d32", 40, 77, 32, 16, 34, 17, 10000, 6),
    ("padded_d24", 37, 83, 24, 12, 20, 10, 0, 61),
]


@pytest.mark.parametrize("extra", [0, SUBPIXEL], ids=["interp", "interp_subpixel"])
@pytest.mark.parametrize("stages", [2, 3])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_frame_interp_vs_oracle_chain(gpu_ready, orc, case, stages, extra):
    from stm_amd import device_api as dev, synth
    name, H, W, D, zd, usd, lsd, variant, seed = case
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + seed)
    p = dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd)
    lib = dev.lib()
    lib.stm_set_agg_variant(variant)
    try:
        dl, dr, out = _run(sbs, p, stages | dev.STAGE_INTERP | extra, H, W)
        dl0, dr0, _ = _run(sbs, p, stages | extra, H, W)  # the same frame without the bit
    finally:
        lib.stm_set_agg_variant(0)
    wl, wr, mux, info = interp_frame(orc, sbs, p, stages, True, subpixel=bool(extra))
    assert np.array_equal(dl, wl) and np.array_equal(dr, wr), name
    if stages == 3:
        assert np.array_equal(out, mux), name
    for side in "lr":  # the case fills something in both views ...
        assert not np.array_equal(info["interp_" + side], info["voted_" + side]), name
    assert not np.array_equal(dl, dl0) and not np.array_equal(dr, dr0), name  # ... and the frame shows it


@pytest.mark.parametrize("stages", [2, 3])
def test_frame_interp_with_hslo_vs_oracle_chain(gpu_ready, orc, stages):
    """stages | 0x400 | 0x100: the chain starts from the oracle's post-HSLO maps and the arms of orc.ca_cross"""
    from stm_amd import device_api as dev, synth
    H, W, D, zd = 48, 100, 16, 8
    sbs, _ = synth.sbs_frame(H, W, D, zd, seed=synth.SEED + 77)
    p = dev.FrameParams(num_disp=D, zero_disp=zd, usd=17, lsd=8)
    dl, dr, out = _run(sbs, p, stages | INTERP | HSLO, H, W)
    dl0, _, _ = _run(sbs, p, stages | HSLO, H, W)
    wl, wr, mux, _ = interp_frame(orc, sbs, p, stages, True, hslo=True)
    assert np.array_equal(dl, wl) and np.array_equal(dr, wr)
    if stages == 3:
        assert np.array_equal(out, mux)
    assert not np.array_equal(dl, dl0)


def test_bud_pair_interp_full_frame(gpu_ready, orc):
    """The real-content bud pair (640 x 384, D = 32; 12 % of the image still marked after voting) through stages 3 | 0x400"""
    from stm_amd import bmp_io, device_api as dev
    g = load_golden("bud_c1_golden")
    D, zd, ad, ce, ucd, lcd, usd, lsd, ts, th, N, angle = [float(x) for x in g["params"]]
    L, R = bmp_io.read_bmp(os.path.join(GOLDEN, "bud_2.bmp")), bmp_io.read_bmp(os.path.join(GOLDEN, "bud_3.bmp"))
    H, W, _ = L.shape
    sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
    p = dev.FrameParams(num_disp=int(D), zero_disp=int(zd), num_views=int(N), angle=angle, ad_coeff=ad, census_coeff=ce,
                        ucd=ucd, lcd=lcd, usd=int(usd), lsd=int(lsd), thresh_s=int(ts), thresh_h=th)
    dl, dr, out = _run(sbs, p, 3 | INTERP, H, W)
    wl, wr, mux, info = interp_frame(orc, sbs, p, 3, True)
    assert np.count_nonzero(info["outl_l"]) > 0.05 * H * W
    assert np.array_equal(dl, wl) and np.array_equal(dr, wr)
    assert np.array_equal(out, mux)


def test_1080p_d64_interp_stage2(gpu_ready, orc):
    """The frame bench.py times (1920 x 1080, D = 64, default parameters) at stages 2 | 0x400."""
    from stm_amd import device_api as dev, synth
    H, W, D, zd = 1080, 1920, 64, 32
    sbs, _ = synth.sbs_frame(H, W, D, zd)
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    dl, dr, _ = _run(sbs, p, 2 | INTERP, H, W)
    wl, wr, _, info = interp_frame(orc, sbs, p, 2, True)
    assert not np.array_equal(info["interp_l"], info["voted_l"])
    assert np.array_equal(dl, wl) and np.array_equal(dr, wr)


def test_interp_without_refinement_is_an_error(gpu_ready):
    """1 | 0x400 has no outlier maps: it fails through stm_last_error before anything runs, the caller's buffers keep their contents"""
    from stm_amd import device_api as dev, synth
    H, W, D, zd = 24, 40, 16, 8
    sbs, _ = synth.sbs_frame(H, W, D, zd)
    p = dev.FrameParams(num_disp=D, zero_disp=zd, usd=17, lsd=8)
    lib = dev.lib()
    lib.stm_set_error_mode(1)
    try:
        lib.stm_last_error()  # clear
        dl, dr, out = _run(sbs, p, 1 | INTERP, H, W, fill=7)
        err = lib.stm_last_error()
    finally:
        lib.stm_set_error_mode(0)
    assert err and b"0x400" in err, err
    assert np.all(dl == 7) and np.all(dr == 7) and np.all(out == 7)


def test_default_path_untouched_by_the_new_bit(gpu_ready, orc):
    """The same frame with 0x400, without it, with it again: without it the result is the oracle's adcensus_stm"""
    from stm_amd import device_api as dev
    H, W, D, zd = 56, 120, 32, 16
    L, R = rand_pair(H, W, 41)
    sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
    p = dev.FrameParams(num_disp=D, zero_disp=zd, usd=17, lsd=8)
    want = orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, D, zd, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                            p.thresh_s, p.thresh_h)
    wl, wr, mux, _ = interp_frame(orc, sbs, p, 3, True)
    runs = [_run(sbs, p, st, H, W) for st in (3 | INTERP, 3, 3 | INTERP, 3)]
    for dl, dr, out in (runs[1], runs[3]):
        assert np.array_equal(dl, want["disp_l"]) and np.array_equal(dr, want["disp_r"])
        assert np.array_equal(out, want["interlaced"])
    for dl, dr, out in (runs[0], runs[2]):
        assert np.array_equal(dl, wl) and np.array_equal(dr, wr) and np.array_equal(out, mux)
    assert not np.array_equal(runs[0][0], runs[1][0])


def test_frame_stream_with_interp(gpu_ready):
    """stm_stream_set_stages(3 | 0x400): every frame of the stream (eager, captured and replayed ones) equals the device frame
    call with the same stages; the setter refuses 0x100, and anything after the first submit"""
    from stm_amd import device_api as dev, synth, video
    H, W, D, zd = 40, 72, 8, 4
    p = dev.FrameParams(num_disp=D, zero_disp=zd, usd=9, lsd=4)
    frames = [synth.sbs_frame(H, W, D, zd, seed=synth.SEED + 500 + k)[0] for k in range(6)]
    lib = dev.lib()
    fs = video.FrameStream(H, W, p)
    lib.stm_set_error_mode(1)
    try:
        lib.stm_last_error()
        assert lib.stm_stream_set_stages(fs._h, 3 | HSLO) == -1
        assert b"stages" in lib.stm_last_error()
        assert lib.stm_stream_set_stages(fs._h, 2 | INTERP) == -1
        assert lib.stm_stream_set_stages(fs._h, 3 | INTERP) == 0
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
            fs.set_stages(3 | INTERP | SUBPIXEL)
        while pending:
            got.append(fs.collect())
            pending -= 1
    finally:
        lib.stm_set_error_mode(0)
        fs.close()
    assert [g[0] for g in got] == list(range(6))
    differs = False
    for k, f in enumerate(frames):
        dl, dr, out = _run(f, p, 3 | INTERP, H, W)
        assert np.array_equal(got[k][1], dl) and np.array_equal(got[k][2], dr) and np.array_equal(got[k][3], out), k
        differs |= not np.array_equal(dl, _run(f, p, 3, H, W)[0])
    assert differs
