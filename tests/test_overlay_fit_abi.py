"""CPU checks of the overlay placement's C boundary (stm_overlay_fit / stm_d_overlay_fit, stm_set_overlay_auto, stm_get_overlay_auto,
stm_stream_set_overlay_auto, stm_stream_overlay_depth): declared, exported, prototyped with the right int / float / pointer kinds,
usable from plain C and C++, and the argument rules -- every refusal happens before anything is launched, so these run without a GPU.
(A frame stream cannot be created without one: the two stream calls' rules -- before stm_stream_set_overlay, after the first submit
-- are in test_gpu_overlay_fit.py.)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "include")
SYMBOLS = ["stm_overlay_fit", "stm_d_overlay_fit", "stm_set_overlay_auto", "stm_get_overlay_auto", "stm_stream_set_overlay_auto",
           "stm_stream_overlay_depth"]
f32p = ctypes.POINTER(ctypes.c_float)
u8p = ctypes.POINTER(ctypes.c_uint8)
INF, NAN = float("inf"), float("nan")
DEFAULT = (0, 20, 1.0, 8, 0.0, 0.0, 1.0, np.float32(0.1))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "stm_hip.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_prototyped(stm):
    from stm_amd import _lib
    declared = set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header()))
    out = subprocess.check_output(["nm", "-D", "--defined-only", stm.LIB_PATH]).decode()
    exported = set(re.findall(r"\bT (stm_[a-z0-9_]+)\b", out))
    for name in SYMBOLS:
        assert name in declared, name
        assert name in exported, name
        assert name in _lib.PROTOS, name


def test_prototypes_match_the_declarations():
    """argument count and the int / float / pointer kind of every argument, read off the header"""
    from stm_amd import _lib
    txt = _header()

    def kind(arg):
        if "*" in arg or "[" in arg:
            return "p"
        return {"int": "i", "float": "f", "double": "d"}[arg.split()[0]]
    ctype_kind = {ctypes.c_int: "i", ctypes.c_float: "f", ctypes.c_double: "d"}
    for name in SYMBOLS:
        m = re.search(r"\b(int|void)\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        kinds = [kind(a.strip()) for a in m.group(2).split(",")]
        args, res = _lib.PROTOS[name]
        assert res is (ctypes.c_int if m.group(1) == "int" else None), name
        got = [ctype_kind.get(a, "p") for a in args]
        assert got == kinds, (name, got, kinds)
    # (disp_l, disp_r, num_rows, num_cols, overlay, ov_rows, ov_cols, x0, y0, view_rows, view_cols, float gain, conv, near_permille,
    #  float margin, pad, float limit_lo, limit_hi, rate_near, rate_far, restart, state[, cut_state])
    assert "".join(ctype_kind.get(a, "p") for a in _lib.PROTOS["stm_overlay_fit"][0]) == "ppiipiiiiiiffififfffip"
    assert "".join(ctype_kind.get(a, "p") for a in _lib.PROTOS["stm_d_overlay_fit"][0]) == "ppiipiiiiiiffififfffipp"
    assert "".join(ctype_kind.get(a, "p") for a in _lib.PROTOS["stm_set_overlay_auto"][0]) == "iififfffp"
    assert "".join(ctype_kind.get(a, "p") for a in _lib.PROTOS["stm_stream_set_overlay_auto"][0]) == "piififfff"


def test_calls_compile_from_plain_c_and_cxx(tmp_path):
    body = ('#include "stm_hip.h"\n'
            'int use(void *s, float *dl, float *dr, const unsigned char *ov, float *state, const int *cut) {\n'
            '    int mode[3];\n'
            '    float v[5], rec[4];\n'
            '    if (stm_set_overlay_auto(1, 20, 1.0f, 8, -30.0f, 10.0f, 1.0f, 0.1f, state) != 0) return -1;\n'
            '    stm_get_overlay_auto(mode, v);\n'
            '    stm_overlay_fit(dl, dr, 1080, 1920, ov, 120, 1920, 0, 900, 1080, 1920, 1.0f, 0.0f, mode[1], v[0], mode[2], v[1], v[2], v[3], v[4], 0, state);\n'
            '    stm_d_overlay_fit(dl, dr, 540, 960, ov, 120, 1920, 0, 900, 1080, 1920, 0.5f, 2.0f, 20, 1.0f, 8, -30.0f, 10.0f, 1.0f, 0.1f, 1, state, cut);\n'
            '    stm_d_overlay_fit(dl, dr, 540, 960, ov, 120, 1920, 0, 900, 1080, 1920, 0.5f, 2.0f, 20, 1.0f, 8, -30.0f, 10.0f, 1.0f, 0.1f, 0, state, 0);\n'
            '    if (stm_stream_set_overlay_auto(s, 1, 20, 1.0f, 8, -30.0f, 10.0f, 1.0f, 0.1f) != 0) return -1;\n'
            '    return stm_stream_overlay_depth(s, rec) + stm_set_overlay_auto(0, 0, 0.0f, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0);\n'
            '}\n')
    c = tmp_path / "t.c"
    c.write_text(body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-c", str(c), "-o", str(tmp_path / "t.o")])
    cpp = tmp_path / "t.cpp"
    cpp.write_text(body)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", INC, "-c", str(cpp), "-o", str(tmp_path / "u.o")])
    und = subprocess.check_output(["nm", "-u", str(tmp_path / "u.o")]).decode()
    for name in SYMBOLS:
        assert re.search(r"\b%s\b" % name, und), name  # C linkage from C++ too


@pytest.fixture
def lib(stm):
    lib = stm.lib()
    lib.stm_set_error_mode(1)
    try:
        yield lib
    finally:
        lib.stm_set_overlay_auto(0, 0, 0.0, 0, 0.0, 0.0, 0.0, 0.0, None)
        lib.stm_set_overlay(0, None, 0, 0, 0, 0, 0.0)
        lib.stm_set_error_mode(0)


def _arm(lib):
    """plant a known message: a later check sees the call's own message or this one, never an earlier call's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


def _auto(lib):
    m = (ctypes.c_int * 3)()
    v = (ctypes.c_float * 5)()
    lib.stm_get_overlay_auto(m, ctypes.cast(v, f32p))
    return (m[0], m[1], v[0], m[2], v[1], v[2], v[3], v[4])


# (near_permille, margin, pad, limit_lo, limit_hi, rate_near, rate_far) that every entry refuses, and the word the message must carry
GOOD7 = (20, 1.0, 8, -30.0, 10.0, 1.0, 0.5)


def _seven(**kw):
    names = ("near_permille", "margin", "pad", "limit_lo", "limit_hi", "rate_near", "rate_far")
    g = dict(zip(names, GOOD7))
    g.update(kw)
    return tuple(g[n] for n in names)


AUTO_RULES = [(_seven(near_permille=-1), b"near_permille"), (_seven(near_permille=500), b"near_permille"),
              (_seven(margin=NAN), b"margin"), (_seven(margin=INF), b"margin"), (_seven(margin=-4096.5), b"margin"),
              (_seven(pad=-1), b"pad"), (_seven(pad=4097), b"pad"),
              (_seven(limit_lo=NAN), b"limit_lo"), (_seven(limit_lo=-INF), b"limit_lo"), (_seven(limit_lo=-4097.0), b"limit_lo"),
              (_seven(limit_hi=NAN), b"limit_hi"), (_seven(limit_hi=INF), b"limit_hi"), (_seven(limit_hi=4096.5), b"limit_hi"),
              (_seven(limit_lo=3.0, limit_hi=2.5), b"limit_lo"),
              (_seven(rate_near=0.0), b"rate_near"), (_seven(rate_near=1.125), b"rate_near"), (_seven(rate_near=NAN), b"rate_near"),
              (_seven(rate_near=-0.5), b"rate_near"),
              (_seven(rate_far=0.0), b"rate_far"), (_seven(rate_far=1.125), b"rate_far"), (_seven(rate_far=NAN), b"rate_far")]


def test_setter_rules_leave_the_setting_readable(lib):
    assert _auto(lib) == DEFAULT  # the default: off
    state = np.zeros(4, np.float32)  # (host memory stands in for the device pointer: the setter only records it)
    assert lib.stm_set_overlay_auto(1, 35, -2.5, 12, -40.0, 7.25, 0.75, 0.125, state.ctypes.data) == 0
    now = (1, 35, -2.5, 12, -40.0, 7.25, 0.75, 0.125)
    assert _auto(lib) == now
    refusals = [((2,) + GOOD7, b"mode"), ((-1,) + GOOD7, b"mode")] + [((1,) + rule, word) for rule, word in AUTO_RULES]
    for args, word in refusals:
        _arm(lib)
        assert lib.stm_set_overlay_auto(*args, state.ctypes.data) == -1, args
        err = lib.stm_last_error()
        assert b"set_overlay_auto:" in err and word in err, (args, err)
        assert _auto(lib) == now, args  # unchanged
    for args in ((1, 0, 4096.0, 0, -4096.0, -4096.0, 1.0, 1.0), (1, 499, -4096.0, 4096, 4096.0, 4096.0, 0.5, 0.25), (1, 20, 0.0, 8, 2.0, 2.0, 1.0, 1.0)):
        assert lib.stm_set_overlay_auto(*args, None) == 0, args
        assert _auto(lib) == args
    assert lib.stm_set_overlay_auto(0, -5, NAN, 99999, NAN, INF, 7.0, -1.0, None) == 0  # mode 0: the other arguments are ignored
    assert _auto(lib) == DEFAULT
    # a setting of its own: stm_set_overlay neither has a mode 2 nor reports this one
    ov = np.zeros((3, 5, 4), np.uint8)
    assert lib.stm_set_overlay_auto(1, *GOOD7, None) == 0
    assert lib.stm_set_overlay(2, ov.ctypes.data, 3, 5, 0, 0, 0.0) == -1
    out, disp = (ctypes.c_int * 5)(), ctypes.c_float(-1.0)
    lib.stm_get_overlay(out, ctypes.byref(disp))
    assert tuple(out) == (0, 0, 0, 0, 0)
    assert (state == 0).all()


# (num_rows, num_cols, ov_rows, ov_cols, x0, y0, view_rows, view_cols, gain, conv) of a stage call
GOOD_STAGE = (8, 12, 3, 5, 1, 2, 8, 12, 1.0, 0.0)


def _stage(**kw):
    names = ("num_rows", "num_cols", "ov_rows", "ov_cols", "x0", "y0", "view_rows", "view_cols", "gain", "conv")
    g = dict(zip(names, GOOD_STAGE))
    g.update(kw)
    return tuple(g[n] for n in names)


STAGE_RULES = [(_stage(num_rows=0), b"num_rows"), (_stage(num_cols=-1), b"num_cols"), (_stage(view_rows=0), b"view_rows"),
               (_stage(view_cols=0), b"view_cols"), (_stage(num_rows=65536, num_cols=32768), b"2^31"),
               (_stage(ov_rows=0), b"ov_rows"), (_stage(ov_rows=65536), b"ov_rows"), (_stage(ov_cols=0), b"ov_cols"),
               (_stage(ov_cols=65536), b"ov_cols"), (_stage(x0=65537), b"x0"), (_stage(x0=-65537), b"x0"), (_stage(y0=65537), b"y0"),
               (_stage(y0=-65537), b"y0"), (_stage(gain=-0.125), b"gain"), (_stage(gain=8.5), b"gain"), (_stage(gain=NAN), b"gain"),
               (_stage(conv=NAN), b"conv"), (_stage(conv=INF), b"conv"), (_stage(conv=4097.0), b"conv")]


def test_stage_rules_are_reported_and_nothing_is_written(lib):
    """both flavours; the state keeps its bits.  (The device flavour is given host memory: no call gets past the screen.)"""
    dl, dr = np.full((8, 12), 3, np.float32), np.full((8, 12), 4, np.float32)
    ov = np.full((3, 5, 4), 9, np.uint8)
    state = np.array([1, NAN, -0.0, 7], np.float32)
    before = state.tobytes()
    cases = [(g[:8] + g[8:] + GOOD7, word) for g, word in STAGE_RULES] + [(GOOD_STAGE + rule, word) for rule, word in AUTO_RULES]
    for dev in (False, True):
        name = b"d_overlay_fit" if dev else b"overlay_fit"
        for args, word in cases:
            _arm(lib)
            if dev:
                lib.stm_d_overlay_fit(dl.ctypes.data, dr.ctypes.data, *args[:2], ov.ctypes.data, *args[2:], 0, state.ctypes.data, None)
            else:
                lib.stm_overlay_fit(dl.ctypes.data_as(f32p), dr.ctypes.data_as(f32p), *args[:2], ov.ctypes.data_as(u8p), *args[2:], 0,
                                    state.ctypes.data_as(f32p))
            err = lib.stm_last_error()
            assert (b" " + name + b":") in (b" " + err).replace(b"\n", b" ") and word in err, (name, args, err)
        _arm(lib)
        if dev:
            lib.stm_d_overlay_fit(dl.ctypes.data, dr.ctypes.data, 8, 12, None, *GOOD_STAGE[2:], *GOOD7, 0, state.ctypes.data, None)
        else:
            lib.stm_overlay_fit(dl.ctypes.data_as(f32p), dr.ctypes.data_as(f32p), 8, 12, None, *GOOD_STAGE[2:], *GOOD7, 0, state.ctypes.data_as(f32p))
        assert b"null" in lib.stm_last_error()
    _arm(lib)
    lib.stm_d_overlay_fit(dl.ctypes.data, dr.ctypes.data, 8, 12, ov.ctypes.data + 2, *GOOD_STAGE[2:], *GOOD7, 0, state.ctypes.data, None)
    assert b"aligned" in lib.stm_last_error()  # the device flavour reads whole words
    assert state.tobytes() == before and (dl == 3).all() and (dr == 4).all() and (ov == 9).all()
    assert _auto(lib) == DEFAULT  # the stage does not touch the thread's setting
