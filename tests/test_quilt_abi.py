"""CPU checks of the quilt's C boundary (stm_set_layout, stm_get_layout, stm_quilt_multiview / stm_d_quilt_multiview,
stm_stream_set_layout): declared, exported, prototyped, usable from plain C and C++, and the argument rules -- every refusal happens
before anything is launched, so these run without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "include")
SYMBOLS = ["stm_set_layout", "stm_get_layout", "stm_quilt_multiview", "stm_d_quilt_multiview", "stm_stream_set_layout",
           "stm_set_quilt_lds_limit"]
u8p = ctypes.POINTER(ctypes.c_uint8)


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
    """argument count and the int / pointer kind of every argument, read off the header"""
    from stm_amd import _lib
    txt = _header()
    for name in SYMBOLS:
        m = re.search(r"\b(int|void)\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        kinds = ["p" if ("*" in arg or "[" in arg) else "i" for arg in (a.strip() for a in m.group(2).split(","))]
        args, res = _lib.PROTOS[name]
        assert res is (ctypes.c_int if m.group(1) == "int" else None), name
        got = ["i" if a is ctypes.c_int else "p" for a in args]
        assert got == kinds, (name, got, kinds)


def test_calls_compile_from_plain_c_and_cxx(tmp_path):
    body = ('#include "stm_hip.h"\n'
            'int use(void *s, unsigned char **views, unsigned char *out) {\n'
            '    int now[5];\n'
            '    if (stm_set_layout(1, 8, 6, 3, 1) != 0) return -1;\n'
            '    stm_get_layout(now);\n'
            '    stm_quilt_multiview(views, out, 48, 8, 6, 3, 1, 1080, 1920, 3360, 3360, 3);\n'
            '    stm_d_quilt_multiview(views, out, 2, 2, 1, 2, 0, 1080, 1920, 1080, 3840, 4);\n'
            '    stm_set_quilt_lds_limit(0);\n'
            '    return stm_stream_set_layout(s, now[0], now[1], now[2], now[3], now[4]);\n'
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
        lib.stm_set_layout(0, 0, 0, 0, 0)
        lib.stm_set_lens(0, 0.0, 0.0, 0.0)
        lib.stm_set_error_mode(0)


def _arm(lib):
    """plant a known message: a later check sees the call's own message or this one, never an earlier call's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


def _layout(lib):
    now = (ctypes.c_int * 5)()
    lib.stm_get_layout(now)
    return tuple(now)


def test_set_layout_rules_leave_the_state_readable(lib):
    assert _layout(lib) == (0, 1, 1, 0, 0)  # the default
    assert lib.stm_set_layout(1, 4, 2, 3, 1) == 0
    assert _layout(lib) == (1, 4, 2, 3, 1)
    for args, word in (((2, 4, 2, 0, 0), b"layout"), ((-1, 4, 2, 0, 0), b"layout"), ((1, 0, 2, 0, 0), b"tiles_x"), ((1, 4, -1, 0, 0), b"tiles_y"),
                       ((1, 4, 2, 4, 0), b"order"), ((1, 4, 2, -1, 0), b"order"), ((1, 4, 2, 0, 2), b"filter"), ((1, 4, 2, 0, -1), b"filter"),
                       ((1, 65536, 1, 0, 0), b"tiles_x")):
        _arm(lib)
        assert lib.stm_set_layout(*args) == -1, args
        err = lib.stm_last_error()
        assert b"set_layout:" in err and word in err, (args, err)
        assert _layout(lib) == (1, 4, 2, 3, 1), args  # unchanged
    for args in ((1, 1, 2, 0, 0), (1, 8, 6, 1, 1), (1, 2, 1, 2, 0)):
        assert lib.stm_set_layout(*args) == 0
        assert _layout(lib) == args
    assert lib.stm_set_layout(0, -5, 99, 7, 7) == 0  # layout 0: the other arguments are ignored
    assert _layout(lib) == (0, 1, 1, 0, 0)


# (num_views, tiles_x, tiles_y, order, filter, in_rows, in_cols, out_rows, out_cols, elem_sz), the word the message must carry
STAGE_RULES = [((8, 4, 2, 0, 0, 0, 8, 8, 8, 3), b"in_rows"), ((8, 4, 2, 0, 0, 8, 8, 8, 0, 3), b"out_cols"), ((8, 4, 2, 0, 0, 8, 8, 8, 8, 2), b"elem_sz"),
               ((1, 1, 1, 0, 0, 8, 8, 8, 8, 3), b"num_views"), ((8, 0, 2, 0, 0, 8, 8, 8, 8, 3), b"tiles_x"), ((8, 4, 0, 0, 0, 8, 8, 8, 8, 3), b"tiles_y"),
               ((8, 4, 2, 4, 0, 8, 8, 8, 8, 3), b"order"), ((8, 4, 2, 0, 2, 8, 8, 8, 8, 3), b"filter"), ((8, 4, 3, 0, 1, 8, 8, 8, 8, 3), b"num_views"),
               ((7, 4, 2, 0, 1, 8, 8, 8, 8, 3), b"num_views"), ((8, 4, 2, 0, 1, 8, 8, 8, 3, 3), b"out_cols"), ((8, 4, 2, 0, 0, 8, 8, 1, 8, 3), b"out_rows"),
               ((2, 2, 1, 0, 1, 8, 1 << 20, 8, 1 << 13, 3), b"out_cols"), ((2, 1, 2, 0, 1, 1 << 20, 8, 1 << 13, 8, 3), b"out_rows")]


def test_stage_rules_are_reported_and_nothing_is_written(lib):
    """both flavours; the output keeps its fill.  (The device flavour is given host memory: no call gets past the screen.)"""
    out = np.full((8, 8, 4), 7, np.uint8)
    views = [np.full((8, 8, 4), 9, np.uint8) for _ in range(8)]
    tab = (u8p * 8)(*[v.ctypes.data_as(u8p) for v in views])
    for rule, word in STAGE_RULES:
        for fn, name in ((lib.stm_quilt_multiview, b"quilt_multiview"), (lib.stm_d_quilt_multiview, b"d_quilt_multiview")):
            _arm(lib)
            if name.startswith(b"d_"):
                fn(ctypes.cast(tab, ctypes.c_void_p), out.ctypes.data, *rule)
            else:
                fn(ctypes.cast(tab, ctypes.POINTER(u8p)), out.ctypes.data_as(u8p), *rule)
            err = lib.stm_last_error()
            assert word in err and (b" " + name + b":") in err.replace(b"\n", b" "), (rule, err)
    assert (out == 7).all()
    assert _layout(lib) == (0, 1, 1, 0, 0)  # the stage does not touch the thread's layout


def _frame(lib, name, rows_out=8, cols_out=12, views=8, stages=3):
    """a frame call with all pointers null: nothing can be launched"""
    rows, wsbs, cols = 8, 24, 12
    tail = (rows, wsbs, cols, rows_out, cols_out, 3, views, 18.0, 8, 4, 10.0, 30.0, 6.0, 20.0, 17, 8, 20, 0.4)
    if name == "stm_d_adcensus_stm":
        lib.stm_d_adcensus_stm(None, None, None, None, *tail, stages)
    elif name == "stm_d_adcensus_stm_t":
        lib.stm_d_adcensus_stm_t(None, None, None, None, *tail, stages, None, None, None, 0.5, 24, 1.5)
    elif name == "stm_d_adcensus_stm_nv12":
        lib.stm_d_adcensus_stm_nv12(None, wsbs, None, wsbs, 0, None, None, None, *tail, stages, None, None, None, None, 0.5, 24, 1.5, None, None)
    elif name == "stm_adcensus_stm":
        lib.stm_adcensus_stm(None, None, None, None, *tail)
    else:
        reduced = (rows, wsbs, cols, rows_out, cols_out, rows // 2, cols // 2, 3, 0.5, views, 18.0, 8, 4, 10.0, 30.0, 6.0, 20.0, 17, 8, 20, 0.4)
        getattr(lib, name)(None, None, None, None, *(reduced + ((3,) if name.endswith("2s") else ())))


FRAME_CALLS = ("stm_d_adcensus_stm", "stm_d_adcensus_stm_t", "stm_d_adcensus_stm_nv12", "stm_adcensus_stm", "stm_adcensus_stm_2",
               "stm_d_adcensus_stm_2", "stm_adcensus_stm_2s", "stm_d_adcensus_stm_2s")


def test_every_frame_call_screens_the_tiling_before_it_launches(lib):
    """null pointers throughout: a call that got past the screen would dereference them"""
    cases = [((1, 4, 2, 0, 1), dict(views=6), None, b"num_views"), ((1, 3, 3, 0, 0), dict(), None, b"num_views"),
             ((1, 8, 1, 0, 1), dict(cols_out=7), None, b"num_cols_out"), ((1, 1, 8, 0, 1), dict(rows_out=7), None, b"num_rows_out"),
             ((1, 4, 2, 0, 1), dict(), (1, 8.0, 1.0, 0.0), b"lens"), ((1, 4, 2, 3, 0), dict(), (3, 7.37, 0.86, 0.3), b"lens")]
    for lo, kw, lens, word in cases:
        assert lib.stm_set_layout(*lo) == 0
        assert lib.stm_set_lens(*(lens or (0, 0.0, 0.0, 0.0))) == 0
        for name in FRAME_CALLS:
            _arm(lib)
            _frame(lib, name, **kw)
            err = lib.stm_last_error()
            assert name[4:].encode() + b":" in err and word in err, (lo, name, err)
        assert _layout(lib) == lo
