"""CPU checks of the packed-input C boundary (stm_set_packing, the four stage calls, stm_stream_set_packing): declared, exported,
prototyped, usable from plain C and C++, and every argument rule reported through stm_last_error before anything is launched or
written -- the screens run on the host, so they are checked here without a GPU (no call below gets past its screen)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "include")
SYMBOLS = ["stm_set_packing", "stm_get_packing", "stm_demux_packed", "stm_d_demux_packed", "stm_demux_nv12_packed", "stm_d_demux_nv12_packed",
           "stm_stream_set_packing"]
u8p = ctypes.POINTER(ctypes.c_uint8)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "stm_hip.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_prototyped(stm):
    from stm_amd import _lib
    declared = set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header()))
    out = subprocess.check_output(["nm", "-D", "--defined-only", stm.LIB_PATH]).decode()
    have = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    for name in SYMBOLS:
        assert name in declared, name
        assert name in have, name
        assert name in _lib.PROTOS, name


def test_prototypes_match_the_declarations():
    from stm_amd import _lib
    txt = _header()
    for name in SYMBOLS:
        m = re.search(r"\b(int|void)\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        kinds = ["p" if "*" in arg else "i" for arg in (a.strip() for a in m.group(2).split(","))]
        args, res = _lib.PROTOS[name]
        assert res is (ctypes.c_int if m.group(1) == "int" else None), name
        assert ["i" if a is ctypes.c_int else "p" for a in args] == kinds, name


def test_calls_compile_from_plain_c_and_cxx(tmp_path):
    body = ('#include "stm_hip.h"\n'
            'int use(void *s, unsigned char *a, unsigned char *b, unsigned char *c, unsigned char *d) {\n'
            '    if (stm_set_packing(1, 0, 1, 0) != 0) return -1;\n'
            '    int now[4];\n'
            '    stm_get_packing(now);\n'
            '    stm_demux_packed(a, b, c, 4, 8, 8, 3, 1, 0, 1, 0);\n'
            '    stm_d_demux_packed(a, b, c, 4, 8, 8, 3, 1, 0, 1, 0);\n'
            '    stm_demux_nv12_packed(a, b, c, 8, d, 8, 4, 8, 8, 3, 0, 1, 0, 1, 0);\n'
            '    stm_d_demux_nv12_packed(a, b, c, 8, d, 8, 4, 8, 8, 3, 0, 1, 0, 1, 0);\n'
            '    return stm_stream_set_packing(s, 1, 0, 1, 0);\n'
            '}\n')
    for src, cc, std, obj in (("t.c", "gcc", "-std=c99", "t.o"), ("t.cpp", "g++", "-std=c++11", "u.o")):
        (tmp_path / src).write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-I", INC, "-c", str(tmp_path / src), "-o", str(tmp_path / obj)])
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
        lib.stm_set_packing(0, 0, 0, 0)
        lib.stm_set_error_mode(0)


def _arm(lib):
    """plant a known message: a later check sees the call's own message or this one, never an earlier call's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


# (num_rows, num_cols_sbs, num_cols_out, elem_sz, packing, swap, filter, gap), the word the message must carry
BGR_RULES = [((8, 24, 12, 3, 4, 0, 0, 0), b"packing"), ((8, 24, 12, 3, -1, 0, 0, 0), b"packing"), ((8, 24, 12, 3, 0, 2, 0, 0), b"swap"),
             ((8, 24, 12, 3, 0, -1, 0, 0), b"swap"), ((8, 24, 12, 3, 1, 0, 2, 0), b"filter"), ((8, 24, 12, 3, 1, 0, -1, 0), b"filter"),
             ((8, 24, 12, 3, 0, 0, 0, -1), b"gap"), ((8, 1 << 26, 12, 3, 0, 0, 0, (1 << 24) + 1), b"gap"),
             ((8, 24, 12, 3, 2, 0, 0, (1 << 24) + 1), b"gap"), ((8, 24, 12, 3, 0, 0, 1, 0), b"filter"), ((8, 24, 12, 3, 2, 1, 1, 0), b"filter"),
             ((8, 24, 11, 3, 1, 0, 0, 0), b"num_cols_out"), ((7, 24, 12, 3, 3, 0, 0, 0), b"num_rows"),
             ((8, 23, 12, 3, 0, 0, 0, 0), b"num_cols_sbs"), ((8, 25, 12, 3, 0, 0, 0, 2), b"num_cols_sbs"),
             ((8, 11, 12, 3, 1, 0, 0, 0), b"num_cols_sbs"), ((8, 13, 12, 3, 1, 1, 1, 2), b"num_cols_sbs"),
             ((8, 11, 12, 3, 2, 0, 0, 0), b"num_cols_sbs"), ((8, 11, 12, 3, 3, 0, 1, 4), b"num_cols_sbs"),
             ((0, 24, 12, 3, 0, 0, 0, 0), b"num_rows"), ((8, 24, 0, 3, 0, 0, 0, 0), b"num_cols_out"), ((8, 24, 12, 2, 0, 0, 0, 0), b"elem_sz")]
# NV12 adds (pitch_y, pitch_uv, matrix) in front
NV12_RULES = [((24, 24, 0) + r, w) for r, w in BGR_RULES] + [
    ((24, 24, 0, 7, 24, 12, 3, 0, 0, 0, 0), b"num_rows"), ((24, 24, 0, 8, 24, 11, 3, 0, 0, 0, 0), b"num_cols_out"),
    ((24, 24, 0, 8, 24, 10, 3, 1, 0, 0, 0), b"num_cols_out"), ((24, 24, 0, 6, 24, 12, 3, 3, 0, 0, 0), b"num_rows"),
    ((24, 24, 0, 8, 24, 8, 3, 0, 0, 0, 3), b"gap"), ((24, 24, 0, 8, 24, 12, 3, 2, 0, 0, 1), b"gap"),
    ((23, 24, 0, 8, 24, 12, 3, 0, 0, 0, 0), b"pitch_y"), ((24, 23, 0, 8, 24, 12, 3, 0, 0, 0, 0), b"pitch_uv"),
    ((25, 25, 0, 8, 25, 12, 3, 0, 0, 0, 0), b"pitch_uv"), ((24, 24, 4, 8, 24, 12, 3, 0, 0, 0, 0), b"matrix"),
    ((24, 24, -1, 8, 24, 12, 3, 1, 1, 1, 0), b"matrix")]


def test_stage_rules_are_reported_and_nothing_is_written(lib):
    """both flavours of both stage calls; the output images keep their fill, the input its bytes.  (The device flavour is given host
    memory: no call gets past the screen, so nothing dereferences it.)"""
    out_l, out_r = np.full((8, 12, 4), 7, np.uint8), np.full((8, 12, 4), 7, np.uint8)
    src = np.full((32, 32, 4), 9, np.uint8)
    ptr = lambda a: a.ctypes.data_as(u8p)  # noqa: E731
    for rule, word in BGR_RULES:
        for fn, name in ((lib.stm_demux_packed, b"demux_packed"), (lib.stm_d_demux_packed, b"d_demux_packed")):
            _arm(lib)
            if name.startswith(b"d_"):
                fn(out_l.ctypes.data, out_r.ctypes.data, src.ctypes.data, *rule)
            else:
                fn(ptr(out_l), ptr(out_r), ptr(src), *rule)
            err = lib.stm_last_error()
            assert word in err and (b" " + name + b":") in err.replace(b"\n", b" "), (rule, err)
    for rule, word in NV12_RULES:
        py, puv, m = rule[:3]
        for fn, name in ((lib.stm_demux_nv12_packed, b"demux_nv12_packed"), (lib.stm_d_demux_nv12_packed, b"d_demux_nv12_packed")):
            _arm(lib)
            if name.startswith(b"d_"):
                fn(out_l.ctypes.data, out_r.ctypes.data, src.ctypes.data, py, src.ctypes.data, puv, *rule[3:7], m, *rule[7:])
            else:
                fn(ptr(out_l), ptr(out_r), ptr(src), py, ptr(src), puv, *rule[3:7], m, *rule[7:])
            err = lib.stm_last_error()
            assert word in err and (b" " + name + b":") in err.replace(b"\n", b" "), (rule, err)
    assert (out_l == 7).all() and (out_r == 7).all() and (src == 9).all()


def test_set_packing_rules(lib):
    for args, word in (((4, 0, 0, 0), b"packing"), ((-1, 0, 0, 0), b"packing"), ((0, 2, 0, 0), b"swap"), ((1, 0, 2, 0), b"filter"),
                       ((1, 0, 0, -2), b"gap"), ((2, 0, 0, (1 << 24) + 1), b"gap"), ((0, 0, 1, 0), b"filter"), ((2, 0, 1, 0), b"filter")):
        _arm(lib)
        assert lib.stm_set_packing(*args) == -1
        err = lib.stm_last_error()
        assert b"set_packing" in err and word in err, (args, err)
    now = (ctypes.c_int * 4)()
    for args in ((0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 1, 7), (2, 0, 0, 45), (2, 1, 0, 1 << 24), (3, 1, 1, 0)):
        _arm(lib)
        assert lib.stm_set_packing(*args) == 0
        assert b"d_filter_median" in lib.stm_last_error()
        lib.stm_get_packing(now)
        assert tuple(now) == args
    # a refused call leaves the thread's packing as it was: (3, 1, 1, 0) still governs the frame call below
    assert lib.stm_set_packing(9, 0, 0, 0) == -1
    lib.stm_get_packing(now)
    assert tuple(now) == (3, 1, 1, 0)
    _arm(lib)
    _frame(lib, "stm_d_adcensus_stm", rows=7)
    assert b"packing 3" in lib.stm_last_error()


FRAME = dict(rows=8, wsbs=24, cols=12)


def _frame(lib, name, rows=8, wsbs=24, cols=12, py=None, puv=None, stages=3):
    """a frame call whose geometry is refused: all pointers null, nothing can be launched"""
    tail = (rows, wsbs, cols, rows, cols, 3, 8, 18.0, 8, 4, 10.0, 30.0, 6.0, 20.0, 17, 8, 20, 0.4)
    if name == "stm_d_adcensus_stm":
        lib.stm_d_adcensus_stm(None, None, None, None, *tail, stages)
    elif name == "stm_d_adcensus_stm_t":
        lib.stm_d_adcensus_stm_t(None, None, None, None, *tail, stages, None, None, None, 0.5, 24, 1.5)
    elif name == "stm_d_adcensus_stm_nv12":
        lib.stm_d_adcensus_stm_nv12(None, py or wsbs, None, puv or wsbs, 0, None, None, None, *tail, stages, None, None, None, None, 0.5, 24, 1.5,
                                    None, None)
    elif name == "stm_adcensus_stm":
        lib.stm_adcensus_stm(None, None, None, None, *tail)
    else:
        reduced = (rows, wsbs, cols, rows, cols, rows // 2, cols // 2, 3, 0.5, 8, 18.0, 8, 4, 10.0, 30.0, 6.0, 20.0, 17, 8, 20, 0.4)
        getattr(lib, name)(None, None, None, None, *(reduced + ((3,) if name.endswith("2s") else ())))


def test_frame_calls_screen_the_packed_geometry(lib):
    # (the thread's packing, the call's geometry, the word)
    cases = [((1, 0, 0, 0), dict(cols=11), b"num_cols"), ((3, 0, 1, 0), dict(rows=7), b"num_rows"),
             ((0, 1, 0, 0), dict(wsbs=23), b"num_cols_sbs"), ((0, 0, 0, 2), dict(wsbs=25), b"num_cols_sbs"),
             ((1, 0, 1, 4), dict(wsbs=15), b"num_cols_sbs"), ((2, 0, 0, 0), dict(wsbs=11), b"num_cols_sbs"),
             ((3, 1, 0, 2), dict(wsbs=11), b"num_cols_sbs")]
    for pk, kw, word in cases:
        assert lib.stm_set_packing(*pk) == 0
        for name in ("stm_d_adcensus_stm", "stm_d_adcensus_stm_t", "stm_d_adcensus_stm_nv12"):
            _arm(lib)
            _frame(lib, name, **kw)
            err = lib.stm_last_error()
            assert name[4:].encode() + b":" in err and word in err, (pk, name, err)
    nv12 = [((1, 0, 0, 0), dict(cols=10), b"num_cols"), ((3, 0, 0, 0), dict(rows=6), b"num_rows"), ((2, 0, 0, 3), dict(), b"gap"),
            ((0, 1, 0, 0), dict(rows=7), b"num_rows"), ((2, 1, 0, 0), dict(py=23), b"pitch_y"), ((1, 0, 1, 0), dict(puv=23), b"pitch_uv")]
    for pk, kw, word in nv12:
        assert lib.stm_set_packing(*pk) == 0
        _arm(lib)
        _frame(lib, "stm_d_adcensus_stm_nv12", **kw)
        err = lib.stm_last_error()
        assert b"d_adcensus_stm_nv12:" in err and word in err, (pk, err)
    # the stage word is still screened under a packing, and 0x4000 is no packing bit
    assert lib.stm_set_packing(1, 0, 0, 0) == 0
    _arm(lib)
    _frame(lib, "stm_d_adcensus_stm", stages=3 | 0x1000)
    assert b"0x1000" in lib.stm_last_error()


def test_calls_without_packing_support_refuse_it(lib):
    names = ("stm_adcensus_stm", "stm_adcensus_stm_2", "stm_d_adcensus_stm_2", "stm_adcensus_stm_2s", "stm_d_adcensus_stm_2s")
    for pk in ((0, 1, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (3, 0, 1, 0), (0, 0, 0, 2)):
        assert lib.stm_set_packing(*pk) == 0
        for name in names:
            _arm(lib)
            _frame(lib, name, wsbs=64)
            err = lib.stm_last_error()
            assert name[4:].encode() + b":" in err and b"packing" in err, (pk, name, err)
