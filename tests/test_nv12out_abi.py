"""CPU checks of the NV12 output's C boundary (stm_set_output, stm_get_output, stm_mux_nv12 / stm_d_mux_nv12, stm_stream_set_output):
declared, exported, prototyped, usable from plain C and C++, and the argument rules -- every refusal happens before anything is
launched, so these run without a GPU.  (A frame stream cannot be created without one: stm_stream_set_output's ordering rules are in
tests/test_gpu_nv12out.py.)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "include")
SYMBOLS = ["stm_set_output", "stm_get_output", "stm_mux_nv12", "stm_d_mux_nv12", "stm_stream_set_output"]
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
            'int use(void *s, unsigned char *surface, unsigned char *img) {\n'
            '    int now[4];\n'
            '    if (stm_set_output(1, 1, 3584, 3392) != 0) return -1;\n'
            '    stm_get_output(now);\n'
            '    stm_mux_nv12(surface, 3584, surface + 3584 * 3392, 3584, img, 3360, 3360, 3, now[1]);\n'
            '    stm_d_mux_nv12(surface, 3840, surface + 3840 * 1080, 3840, img, 1080, 3840, 4, 0);\n'
            '    return stm_stream_set_output(s, now[0], now[1]);\n'
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
        lib.stm_set_output(0, 0, 0, 0)
        lib.stm_set_layout(0, 0, 0, 0, 0)
        lib.stm_set_error_mode(0)


def _arm(lib):
    """plant a known message: a later check sees the call's own message or this one, never an earlier call's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


def _output(lib):
    now = (ctypes.c_int * 4)()
    lib.stm_get_output(now)
    return tuple(now)


def test_set_output_rules_leave_the_state_readable(lib):
    assert _output(lib) == (0, 0, 0, 0)  # the default
    assert lib.stm_set_output(1, 3, 80, 48) == 0
    assert _output(lib) == (1, 3, 80, 48)
    for args, word in (((2, 0, 0, 0), b"format"), ((-1, 0, 0, 0), b"format"), ((1, 4, 0, 0), b"matrix"), ((1, -1, 0, 0), b"matrix"),
                       ((1, 0, -1, 0), b"pitch"), ((1, 0, 0, -1), b"uv_row"), ((1, 0, -(1 << 31), 0), b"pitch")):
        _arm(lib)
        assert lib.stm_set_output(*args) == -1, args
        err = lib.stm_last_error()
        assert b"set_output:" in err and word in err, (args, err)
        assert _output(lib) == (1, 3, 80, 48), args  # unchanged
    for args in ((1, 0, 0, 0), (1, 2, 4096, 0), (1, 1, 0, 1088)):
        assert lib.stm_set_output(*args) == 0
        assert _output(lib) == args
    assert lib.stm_set_output(0, 9, -5, -7) == 0  # format 0: the other arguments are ignored
    assert _output(lib) == (0, 0, 0, 0)


# (pitch_y, pitch_uv, num_rows, num_cols, elem_sz, matrix), the word the message must carry
STAGE_RULES = [((8, 8, 0, 8, 3, 0), b"num_rows"), ((8, 8, 8, 0, 3, 0), b"num_cols"), ((8, 8, 8, 8, 2, 0), b"elem_sz"),
               ((8, 8, 7, 8, 3, 0), b"num_rows"), ((8, 8, 8, 7, 3, 0), b"num_cols"), ((8, 8, 1, 8, 3, 0), b"num_rows"),
               ((7, 8, 8, 8, 3, 0), b"pitch_y"), ((8, 7, 8, 8, 3, 0), b"pitch_uv"), ((8, 8, 8, 8, 3, 4), b"matrix"),
               ((8, 8, 8, 8, 3, -1), b"matrix"), ((-8, 8, 8, 8, 4, 0), b"pitch_y")]


def test_stage_rules_are_reported_and_nothing_is_written(lib):
    """both flavours; the planes keep their fill.  (The device flavour is given host memory: no call gets past the screen.)"""
    y = np.full((8, 8), 7, np.uint8)
    uv = np.full((4, 8), 9, np.uint8)
    img = np.full((8, 8, 4), 11, np.uint8)
    for rule, word in STAGE_RULES:
        py, puv = rule[:2]
        for fn, name in ((lib.stm_mux_nv12, b"mux_nv12"), (lib.stm_d_mux_nv12, b"d_mux_nv12")):
            _arm(lib)
            if name.startswith(b"d_"):
                fn(y.ctypes.data, py, uv.ctypes.data, puv, img.ctypes.data, *rule[2:])
            else:
                fn(y.ctypes.data_as(u8p), py, uv.ctypes.data_as(u8p), puv, img.ctypes.data_as(u8p), *rule[2:])
            err = lib.stm_last_error()
            assert word in err and (b" " + name + b":") in err.replace(b"\n", b" "), (rule, err)
    assert (y == 7).all() and (uv == 9).all() and (img == 11).all()
    assert _output(lib) == (0, 0, 0, 0)  # the stage does not touch the thread's format


def _frame(lib, name, rows_out=8, cols_out=16, views=8, stages=3):
    """a frame call with all pointers null: nothing can be launched"""
    rows, wsbs, cols = 8, 24, 12
    tail = (rows, wsbs, cols, rows_out, cols_out, 3, views, 18.0, 8, 4, 10.0, 30.0, 6.0, 20.0, 17, 8, 20, 0.4)
    reduced = (rows, wsbs, cols, rows_out, cols_out, rows // 2, cols // 2, 3, 0.5, views, 18.0, 8, 4, 10.0, 30.0, 6.0, 20.0, 17, 8, 20, 0.4)
    hist3, hist4 = (None, None, None, 0.5, 24, 1.5), (None, None, None, None, 0.5, 24, 1.5, None, None)
    if name == "stm_d_adcensus_stm":
        lib.stm_d_adcensus_stm(None, None, None, None, *tail, stages)
    elif name == "stm_d_adcensus_stm_t":
        lib.stm_d_adcensus_stm_t(None, None, None, None, *tail, stages, *hist3)
    elif name == "stm_d_adcensus_stm_nv12":
        lib.stm_d_adcensus_stm_nv12(None, wsbs, None, wsbs, 0, None, None, None, *tail, stages, *hist4)
    elif name == "stm_adcensus_stm":
        lib.stm_adcensus_stm(None, None, None, None, *tail)
    elif name == "stm_d_adcensus_stm_2t":
        lib.stm_d_adcensus_stm_2t(None, None, None, None, *reduced, stages, *hist3)
    elif name == "stm_d_adcensus_stm_2nv12":
        lib.stm_d_adcensus_stm_2nv12(None, wsbs, None, wsbs, 0, None, None, None, *reduced, stages, *hist4)
    else:
        getattr(lib, name)(None, None, None, None, *(reduced + ((stages,) if name.endswith("2s") else ())))


FRAME_CALLS = ("stm_d_adcensus_stm", "stm_d_adcensus_stm_t", "stm_d_adcensus_stm_nv12", "stm_adcensus_stm", "stm_adcensus_stm_2",
               "stm_d_adcensus_stm_2", "stm_adcensus_stm_2s", "stm_d_adcensus_stm_2s", "stm_d_adcensus_stm_2t", "stm_d_adcensus_stm_2nv12")


def test_every_frame_call_screens_the_format_before_it_launches(lib):
    """null pointers throughout: a call that got past the screen would dereference them.  (layout, output, sizes, the word)"""
    quilt = (1, 4, 2, 0, 1)
    cases = [((0, 1, 1, 0, 0), (1, 0, 0, 0), dict(), b"quilts only"),                    # layout 0
             (quilt, (1, 0, 0, 0), dict(rows_out=9), b"num_rows_out"),                   # an odd output size
             (quilt, (1, 1, 0, 0), dict(cols_out=17), b"num_cols_out"),
             (quilt, (1, 2, 0, 0), dict(cols_out=12), b"tile width"),                    # 12 / 4 = 3
             (quilt, (1, 3, 0, 0), dict(rows_out=6), b"tile height"),                    # 6 / 2 = 3
             (quilt, (1, 0, 15, 0), dict(), b"pitch"), (quilt, (1, 0, 0, 7), dict(), b"uv_row")]
    for lo, out, kw, word in cases:
        assert lib.stm_set_layout(*lo) == 0 and lib.stm_set_output(*out) == 0
        for name in FRAME_CALLS:
            _arm(lib)
            _frame(lib, name, **kw)
            err = lib.stm_last_error()
            assert name[4:].encode() + b":" in err and word in err, (lo, out, name, err)
        assert _output(lib) == out



# ----------------------------------------------------------------------------- the tool's option
def test_stm_video_refuses_malformed_nv12_out_options(capsys):
    """--nv12-out needs --quilt and a matrix in 0 .. 3 (usage and -1, nothing read)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("stm_video", os.path.join(ROOT, "tools", "stm_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for tail in (["--nv12-out", "0"], ["--quilt", "4", "2", "3", "1", "--nv12-out"], ["--quilt", "4", "2", "3", "1", "--nv12-out", "4"],
                 ["--quilt", "4", "2", "3", "1", "--nv12-out", "x"]):
        assert mod.main(["stm_video"] + ["x"] * 16 + tail) == -1, tail
        assert "--nv12-out MATRIX" in capsys.readouterr().out
