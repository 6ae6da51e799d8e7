"""The reduced-resolution frame for frame sequences (stm_d_adcensus_stm_2t, stm_d_adcensus_stm_2nv12, stm_demux_sbs_low and its
NV12 twin, stm_stream_set_match_size): the definition as a composition of the oracle's stages that the GPU tests
(test_gpu_front_low.py, test_gpu_reduced_stream.py) compare against bit for bit, tied to the oracle's adcensus_stm_2; the new C
symbols; and the argument rules that need no device -- every refused call returns with stm_last_error naming the call and writes
nothing.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_subpixel_ref import _P
from test_temporal_ref import ALPHA, THRESH_COLOR, THRESH_DISP, halves, temporal_ref
from test_upsample_ref import FRAMES, LINEAR_WARP, render_ref, upsample_frame

TEMPORAL = 0x2000
INC = os.path.join(ROOT, "include")


# ----------------------------------------------------------------------------- the definition
def census32(orc, img):
    """the 32 bits of the census transform that stm_k_census32 keeps: the low word of the oracle's (window rows -1, +1, +2, +3)"""
    return (orc.census(orc.grey(np.ascontiguousarray(img))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def reduced_front_of_views(orc, L, R, h, w):
    """(low_l, low_r, census_l, census_r) of two split images: the oracle's bilinear reduction of each view, and census32 of it"""
    low_l, low_r = orc.tx_scale_bilinear(L, h, w), orc.tx_scale_bilinear(R, h, w)
    return low_l, low_r, census32(orc, low_l), census32(orc, low_r)


def reduced_front_ref(orc, sbs, W, h, w):
    """What stm_demux_sbs_low returns for a side-by-side frame uint8 [H][Wsbs][E], Wsbs >= 2 W: (img_l, img_r, low_l, low_r,
    census_l, census_r); bytes past a pixel's third are 0"""
    L, R = orc.demux_sbs(np.ascontiguousarray(sbs), W)
    return (L, R) + reduced_front_of_views(orc, L, R, h, w)


def reduced_frame_ref(orc, sbs, p, h, w, disp_scale, extra_bits=0, hist=None, out_rows=None, out_cols=None,
                      temporal=(ALPHA, THRESH_COLOR, THRESH_DISP)):
    """The reduced-resolution frame: test_upsample_ref.upsample_frame up to the full-size maps, the temporal step on those maps
    with the full-size views (hist = (previous side-by-side frame, previous disp_l, previous disp_r), or None), then the
    full-size render.  Returns (disp_l, disp_r, interlaced)."""
    H, Wsbs, _ = sbs.shape
    W = Wsbs // 2
    dl, dr, _, info = upsample_frame(orc, sbs, p, h, w, disp_scale, extra_bits & ~TEMPORAL, render=False)
    L, R = info["img_l"], info["img_r"]
    if (extra_bits & TEMPORAL) and hist is not None:
        Lp, Rp = halves(hist[0])
        dl, dr = temporal_ref(dl, hist[1], L, Lp, *temporal), temporal_ref(dr, hist[2], R, Rp, *temporal)
    mux = render_ref(orc, L, R, dl, dr, p, bool(extra_bits & LINEAR_WARP), out_rows or H, out_cols or W)
    return dl, dr, mux


def frame_case(k, D=16, zd=8):
    """(sbs, p, h, w, disp_scale) of FRAMES[k]: the shared inputs of the frame tests"""
    from stm_amd import synth
    H, W, h, w, dseed = FRAMES[k]
    sbs, _ = synth.sbs_frame(H, W, 2 * D, 2 * zd, seed=synth.SEED + dseed)
    return sbs, _P(D, zd, usd=9, lsd=4), h, w, float(w) / float(W)


@pytest.mark.parametrize("k", [0, 1], ids=["48x100", "37x83"])
def test_reduced_frame_ref_is_the_oracles_reduced_frame(orc, k):
    """without history and extra bits reduced_frame_ref is orc.adcensus_stm_2 element for element; the temporal bit without a
    history changes nothing; with one it does"""
    sbs, p, h, w, scale = frame_case(k)
    H, W = sbs.shape[0], sbs.shape[1] // 2
    want = orc.adcensus_stm_2(sbs, H, W, h, w, scale, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd,
                              p.usd, p.lsd, p.thresh_s, p.thresh_h)
    dl, dr, mux = reduced_frame_ref(orc, sbs, p, h, w, scale)
    assert np.array_equal(dl, want["disp_l"]) and np.array_equal(dr, want["disp_r"]) and np.array_equal(mux, want["interlaced"])
    tl, tr, tmux = reduced_frame_ref(orc, sbs, p, h, w, scale, TEMPORAL)
    assert np.array_equal(tl, dl) and np.array_equal(tr, dr) and np.array_equal(tmux, mux)
    prev = (sbs, (dl + np.float32(1)).astype(np.float32), (dr - np.float32(1)).astype(np.float32))  # inside both gates everywhere
    hl, hr, _ = reduced_frame_ref(orc, sbs, p, h, w, scale, TEMPORAL, hist=prev)
    assert np.allclose(hl, dl + 0.5, rtol=0, atol=1e-5) and np.allclose(hr, dr - 0.5, rtol=0, atol=1e-5)  # alpha = 0.5 of the way


def test_reduced_front_ref_clamps_inside_each_eye(orc):
    """the reduction of the left view never sees the right view: changing the right half leaves low_l and census_l as they were"""
    rng = np.random.RandomState(3)
    sbs = rng.randint(0, 256, size=(12, 40, 3)).astype(np.uint8)
    a = reduced_front_ref(orc, sbs, 20, 7, 9)
    other = sbs.copy()
    other[:, 20:] = 255 - other[:, 20:]
    b = reduced_front_ref(orc, other, 20, 7, 9)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[4]) and not np.array_equal(a[3], b[3])
    assert a[4].dtype == np.uint32 and a[2].shape == (7, 9, 3)


# ----------------------------------------------------------------------------- the C boundary
SYMBOLS = {"stm_d_adcensus_stm_2t": 32, "stm_d_adcensus_stm_2nv12": 39, "stm_demux_sbs_low": 13, "stm_d_demux_sbs_low": 13,
           "stm_demux_nv12_low": 17, "stm_d_demux_nv12_low": 17, "stm_stream_set_match_size": 4}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "stm_hip.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_prototyped(stm):
    from stm_amd import _lib
    txt = _header()
    out = subprocess.check_output(["nm", "-D", "--defined-only", stm.LIB_PATH]).decode()
    have = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\b(int|void)\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        kinds = ["p" if "*" in arg else "n" for arg in (a.strip() for a in m.group(2).split(","))]
        assert len(kinds) == nargs, (name, len(kinds))
        assert name in have, name
        args, res = _lib.PROTOS[name]
        assert res is (ctypes.c_int if m.group(1) == "int" else None), name
        assert ["n" if a in (ctypes.c_int, ctypes.c_float) else "p" for a in args] == kinds, name


def test_python_surface_exists(stm):
    from stm_amd import device_api as dev, host_api, video
    for name in ("d_adcensus_stm_2t", "d_adcensus_stm_2nv12", "d_demux_sbs_low", "d_demux_nv12_low"):
        assert callable(getattr(dev, name)), name
    assert callable(host_api.demux_sbs_low) and callable(video.FrameStream.set_match_size)


@pytest.fixture
def lib(stm):
    lib = stm.lib()
    lib.stm_set_error_mode(1)
    try:
        yield lib
    finally:
        lib.stm_set_packing(0, 0, 0, 0)
        lib.stm_set_error_mode(0)


def _arm(lib):
    """plant a known message: a later check sees the call's own message or this one, never an earlier call's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


GEOM = dict(rows=8, wsbs=24, cols=12, h=4, w=6, elem_sz=3)


def _call(lib, name, outs, stages=3, hist=None, imgs=(None, None), alpha=0.5, color=24, tdisp=1.5, py=None, puv=None, matrix=0, **kw):
    """a reduced frame call that its screen refuses.  outs: host arrays standing in for (disp_l, disp_r, interlaced): no call gets
    past the screen, so nothing dereferences them"""
    g = dict(GEOM, **kw)
    a = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    geom = (g["rows"], g["wsbs"], g["cols"], g["rows"], g["cols"], g["h"], g["w"], g["elem_sz"], 0.5)
    tail = (8, 18.0, 8, 4, 10.0, 30.0, 6.0, 20.0, 17, 8, 20, 0.4, stages)
    if name == "stm_d_adcensus_stm_2t":
        hist = hist or (None, None, None)
        lib.stm_d_adcensus_stm_2t(None, a(outs[0]), a(outs[1]), a(outs[2]), *geom, *tail, a(hist[0]), a(hist[1]), a(hist[2]), alpha, color, tdisp)
    else:
        hist = hist or (None, None, None, None)
        lib.stm_d_adcensus_stm_2nv12(None, py or g["wsbs"], None, puv or g["wsbs"], matrix, a(outs[0]), a(outs[1]), a(outs[2]), *geom, *tail,
                                     a(hist[0]), a(hist[1]), a(hist[2]), a(hist[3]), alpha, color, tdisp, a(imgs[0]), a(imgs[1]))


@pytest.mark.parametrize("name", ["stm_d_adcensus_stm_2t", "stm_d_adcensus_stm_2nv12"])
def test_frame_calls_screen_their_arguments(lib, name):
    outs = [np.full((8, 12), 7, np.float32), np.full((8, 12), 7, np.float32), np.full((8, 12, 3), 7, np.uint8)]
    m1, m2 = np.full((8, 12), 3, np.float32), np.full((8, 12), 3, np.float32)
    i1, i2, i3, i4 = (np.full((8, 12, 3), 5, np.uint8) for _ in range(4))
    nv = name.endswith("nv12")
    half = (None, m1, m2, None) if nv else (i1, m1, None)
    alias = (i3, i4, outs[0], m2) if nv else (i1, outs[1], m2)
    cases = [(dict(stages=2), b"stages"), (dict(stages=1 | 0x2000), b"stages"), (dict(stages=0x1003 & ~3), b"stages"),
             (dict(stages=3 | 0x300), b"0x200"), (dict(stages=3 | 0x4000), b"stages"), (dict(stages=3 | 0x8000), b"stages"),
             (dict(stages=3 | 0x10000), b"stages"), (dict(stages=3 | 0x2000, hist=half, imgs=(i1, i2)), b"history"),
             (dict(stages=3 | 0x2000, hist=alias, imgs=(i1, i2)), b"alias"), (dict(stages=3 | 0x2000, alpha=1.5, imgs=(i1, i2)), b"alpha"),
             (dict(stages=3 | 0x2000, color=766, imgs=(i1, i2)), b"thresh_color"), (dict(stages=3 | 0x2000, tdisp=-1.0, imgs=(i1, i2)), b"thresh_disp"),
             (dict(h=0), b"num_rows_disp"), (dict(w=0), b"num_cols_disp"), (dict(w=-3), b"num_cols_disp"), (dict(rows=0), b"num_rows"),
             (dict(cols=0), b"num_cols"), (dict(elem_sz=2), b"elem_sz")]
    if nv:
        cases += [(dict(rows=7), b"num_rows"), (dict(cols=11), b"num_cols"), (dict(wsbs=23), b"num_cols_sbs"), (dict(py=23), b"pitch_y"),
                  (dict(puv=23), b"pitch_uv"), (dict(matrix=4), b"matrix"), (dict(imgs=(i1, None)), b"d_img_l"),
                  (dict(stages=3 | 0x2000), b"d_img_l")]
    else:
        cases += [(dict(stages=3 | 0x2000, hist=(i1, m1, m2), wsbs=23), b"num_cols_sbs")]
    for kw, word in cases:
        _arm(lib)
        _call(lib, name, outs, **kw)
        err = lib.stm_last_error()
        assert (name[4:].encode() + b":") in err and word in err, (kw, err)
    for pk in ((0, 1, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (3, 0, 1, 0), (0, 0, 0, 2)):
        assert lib.stm_set_packing(*pk) == 0
        _arm(lib)
        _call(lib, name, outs, wsbs=64)
        err = lib.stm_last_error()
        assert (name[4:].encode() + b":") in err and b"packing" in err, (pk, err)
    lib.stm_set_packing(0, 0, 0, 0)
    assert all((o == 7).all() for o in outs) and (m1 == 3).all() and (m2 == 3).all() and all((i == 5).all() for i in (i1, i2, i3, i4))


def test_2s_keeps_rejecting_the_temporal_bit(lib):
    _arm(lib)
    lib.stm_d_adcensus_stm_2s(None, None, None, None, 8, 24, 12, 8, 12, 4, 6, 3, 0.5, 8, 18.0, 8, 4, 10.0, 30.0, 6.0, 20.0, 17, 8, 20, 0.4, 3 | 0x2000)
    err = lib.stm_last_error()
    assert b"d_adcensus_stm_2s:" in err and b"stages" in err and b"0x2000" not in err.split(b"must be")[1]


def test_front_stage_calls_screen_their_arguments(lib):
    """both flavours of both stage calls; the outputs keep their fill"""
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    il, ir = np.full((8, 12, 4), 7, np.uint8), np.full((8, 12, 4), 7, np.uint8)
    ll, lr = np.full((4, 6, 4), 7, np.uint8), np.full((4, 6, 4), 7, np.uint8)
    cl, cr = np.full((4, 6), 7, np.uint32), np.full((4, 6), 7, np.uint32)
    src = np.full((16, 32, 4), 9, np.uint8)
    # (num_rows, num_cols_sbs, num_cols, num_rows_disp, num_cols_disp, elem_sz), census planes given (left, right), the word
    rules = [((0, 24, 12, 4, 6, 3), (1, 1), b"num_rows"), ((8, 0, 12, 4, 6, 3), (1, 1), b"num_cols_sbs"), ((8, 24, 0, 4, 6, 3), (1, 1), b"num_cols"),
             ((8, 24, 12, 0, 6, 3), (1, 1), b"num_rows_disp"), ((8, 24, 12, 4, -1, 3), (1, 1), b"num_cols_disp"),
             ((8, 24, 12, 4, 6, 2), (1, 1), b"elem_sz"), ((8, 24, 12, 4, 6, 3), (1, 0), b"census"), ((8, 24, 12, 4, 6, 3), (0, 1), b"census")]
    nv_rules = [((24, 24, 0) + r, c, wd) for r, c, wd in rules] + [
        ((24, 24, 0, 7, 24, 12, 4, 6, 3), (1, 1), b"num_rows"), ((24, 24, 0, 8, 24, 11, 4, 6, 3), (0, 0), b"num_cols"),
        ((24, 24, 0, 8, 23, 12, 4, 6, 3), (1, 1), b"num_cols_sbs"), ((23, 24, 0, 8, 24, 12, 4, 6, 3), (1, 1), b"pitch_y"),
        ((24, 23, 0, 8, 24, 12, 4, 6, 3), (1, 1), b"pitch_uv"), ((24, 24, 4, 8, 24, 12, 4, 6, 3), (1, 1), b"matrix")]
    for rule, cen, word in rules:
        for host in (True, False):
            name = b"demux_sbs_low" if host else b"d_demux_sbs_low"
            _arm(lib)
            if host:
                lib.stm_demux_sbs_low(il.ctypes.data_as(u8p), ir.ctypes.data_as(u8p), ll.ctypes.data_as(u8p), lr.ctypes.data_as(u8p),
                                      cl.ctypes.data_as(u32p) if cen[0] else None, cr.ctypes.data_as(u32p) if cen[1] else None,
                                      src.ctypes.data_as(u8p), *rule)
            else:
                lib.stm_d_demux_sbs_low(il.ctypes.data, ir.ctypes.data, ll.ctypes.data, lr.ctypes.data, cl.ctypes.data if cen[0] else None,
                                        cr.ctypes.data if cen[1] else None, src.ctypes.data, *rule)
            err = lib.stm_last_error()
            assert word in err and (b" " + name + b":") in err.replace(b"\n", b" "), (rule, err)
    for rule, cen, word in nv_rules:
        py, puv, m = rule[:3]
        for host in (True, False):
            name = b"demux_nv12_low" if host else b"d_demux_nv12_low"
            _arm(lib)
            if host:
                lib.stm_demux_nv12_low(il.ctypes.data_as(u8p), ir.ctypes.data_as(u8p), ll.ctypes.data_as(u8p), lr.ctypes.data_as(u8p),
                                       cl.ctypes.data_as(u32p) if cen[0] else None, cr.ctypes.data_as(u32p) if cen[1] else None,
                                       src.ctypes.data_as(u8p), py, src.ctypes.data_as(u8p), puv, *rule[3:], m)
            else:
                lib.stm_d_demux_nv12_low(il.ctypes.data, ir.ctypes.data, ll.ctypes.data, lr.ctypes.data, cl.ctypes.data if cen[0] else None,
                                         cr.ctypes.data if cen[1] else None, src.ctypes.data, py, src.ctypes.data, puv, *rule[3:], m)
            err = lib.stm_last_error()
            assert word in err and (b" " + name + b":") in err.replace(b"\n", b" "), (rule, err)
    assert all((a == 7).all() for a in (il, ir, ll, lr, cl, cr)) and (src == 9).all()
