"""CPU checks of the vertical alignment's C boundary (stm_set_align, stm_set_align_auto, stm_get_align, the four stage calls and the
three frame-stream calls): declared, exported, prototyped, usable from plain C and C++, and the argument screening of every call
that screens before it touches the device (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "include")
SYMBOLS = ["stm_set_align", "stm_set_align_auto", "stm_get_align", "stm_align_rows", "stm_d_align_rows", "stm_align_fit", "stm_d_align_fit",
           "stm_stream_set_align", "stm_stream_set_align_auto", "stm_stream_align"]
NAN, INF = float("nan"), float("inf")
u8p, f32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_float)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "stm_hip.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_prototyped(stm):
    from stm_amd import _lib
    declared = set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header()))
    lib = ctypes.CDLL(stm.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOS, name


def test_prototypes_match_the_declarations():
    """argument count and the int / float / pointer kind of every argument, read off the header"""
    from stm_amd import _lib
    txt = _header()
    for name in SYMBOLS:
        m = re.search(r"\b(int|void)\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        kinds = []
        for arg in m.group(2).split(","):
            arg = arg.strip()
            kinds.append("p" if ("*" in arg or "[" in arg) else ("f" if arg.startswith("float") else "i"))
        args, res = _lib.PROTOS[name]
        assert res is (ctypes.c_int if m.group(1) == "int" else None), name
        got = ["f" if a is ctypes.c_float else ("i" if a is ctypes.c_int else "p") for a in args]
        assert got == kinds, (name, got, kinds)


def test_calls_compile_from_plain_c_and_cxx(tmp_path):
    body = ('#include "stm_hip.h"\n'
            'int use(void *s, unsigned char *o, const unsigned char *l, const unsigned char *r, float *st, int *n, unsigned int *w) {\n'
            '    int m[2]; float v[4], out[3];\n'
            '    if (stm_set_align_auto(16, 1.0f, st) != 0) return -1;\n'
            '    if (stm_set_align(2, 0.0f, 0.0f, 0.0f) != 0) return -1;\n'
            '    stm_get_align(m, v);\n'
            '    stm_align_rows(o, l, 4, 8, 3, 1.5f, 0.0f, 0.0f);\n'
            '    stm_d_align_rows(o, l, 4, 8, 3, 1.5f, 0.0f, 0.0f);\n'
            '    if (stm_align_fit(l, r, 4, 8, 3, 16, 1.0f, st) < 0) return -1;\n'
            '    stm_d_align_fit(l, r, 4, 8, 3, 16, 1.0f, st, n, w, w);\n'
            '    if (stm_stream_set_align_auto(s, 16, 0.25f) != 0) return -1;\n'
            '    if (stm_stream_set_align(s, 2, 0.0f, 0.0f, 0.0f) != 0) return -1;\n'
            '    return stm_stream_align(s, out);\n'
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
        lib.stm_set_align_auto(16, 1.0, None)
        lib.stm_set_align(0, 0.0, 0.0, 0.0)
        lib.stm_set_error_mode(0)


def _arm(lib):
    """plant a known message: a later check sees the call's own message or this one, never an earlier call's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


def _setting(lib):
    m = (ctypes.c_int * 2)(-1, -1)
    v = (ctypes.c_float * 4)(-1.0, -1.0, -1.0, -1.0)
    lib.stm_get_align(m, ctypes.cast(v, f32p))
    return m[0], v[0], v[1], v[2], m[1], v[3]


def test_get_align_defaults(lib):
    assert _setting(lib) == (0, 0.0, 0.0, 0.0, 16, 1.0)


def test_set_align_rules_leave_the_setting_unchanged(lib):
    assert lib.stm_set_align(1, 2.5, 0.25, -0.5) == 0
    assert _setting(lib) == (1, 2.5, 0.25, -0.5, 16, 1.0)
    for k, word in enumerate((b" a ", b" b ", b" c ")):
        for bad in (NAN, INF, -INF):
            args = [1.0, 0.5, 0.25]
            args[k] = bad
            _arm(lib)
            assert lib.stm_set_align(1, *args) == -1, args
            msg = lib.stm_last_error()
            assert b"\nset_align:" in msg and word in msg and b"finite" in msg, (args, msg)
            assert _setting(lib) == (1, 2.5, 0.25, -0.5, 16, 1.0)
    for mode in (-1, 3, 9):
        _arm(lib)
        assert lib.stm_set_align(mode, 0.0, 0.0, 0.0) == -1
        assert b"mode" in lib.stm_last_error()
        assert _setting(lib) == (1, 2.5, 0.25, -0.5, 16, 1.0)
    # modes 0 and 2 ignore the field and read back zeros; the automatic parameters are kept across the modes
    assert lib.stm_set_align_auto(7, 0.5, None) == 0
    assert lib.stm_set_align(2, NAN, INF, 3.0) == 0
    assert _setting(lib) == (2, 0.0, 0.0, 0.0, 7, 0.5)
    assert lib.stm_set_align(0, NAN, 1.0, 1.0) == 0
    assert _setting(lib) == (0, 0.0, 0.0, 0.0, 7, 0.5)


def test_set_align_auto_rules(lib):
    assert lib.stm_set_align_auto(32, 1.0, None) == 0 and lib.stm_set_align_auto(1, 1.0e-6, None) == 0  # the edges are accepted
    assert lib.stm_set_align_auto(9, 0.25, None) == 0
    for (radius, rate), word in [((0, 0.5), b"radius"), ((33, 0.5), b"radius"), ((-4, 0.5), b"radius"), ((8, 0.0), b"rate"),
                                 ((8, 1.5), b"rate"), ((8, -0.5), b"rate"), ((8, NAN), b"rate"), ((8, INF), b"rate")]:
        _arm(lib)
        assert lib.stm_set_align_auto(radius, rate, None) == -1, (radius, rate)
        msg = lib.stm_last_error()
        assert b"\nset_align_auto:" in msg and word in msg, msg
        assert _setting(lib)[4:] == (9, 0.25)


def test_python_setters_raise_and_read_back(lib):
    from stm_amd import device_api as dev
    dev.set_align_auto(12, 0.5)
    dev.set_align(1, 1.25, 0.5, -0.25)
    assert dev.get_align() == (1, 1.25, 0.5, -0.25, 12, 0.5)
    with pytest.raises(ValueError, match="finite"):
        dev.set_align(1, NAN, 0.0, 0.0)
    with pytest.raises(ValueError, match="radius"):
        dev.set_align_auto(40, 0.5)
    assert dev.get_align() == (1, 1.25, 0.5, -0.25, 12, 0.5)
    dev.set_align(0)
    assert dev.get_align()[0] == 0


@pytest.mark.parametrize("name", ["stm_align_rows", "stm_d_align_rows"])
def test_align_rows_rules(lib, name):
    """both flavours refuse before anything is launched or written: out keeps its bytes"""
    fn = getattr(lib, name)
    rows, cols, E = 2, 5, 3
    img = np.arange(rows * cols * E, dtype=np.uint8).reshape(rows, cols, E)
    out = np.full((rows, cols, E), 77, np.uint8)
    dev = name == "stm_d_align_rows"
    po = out.ctypes.data if dev else out.ctypes.data_as(u8p)
    pi = img.ctypes.data if dev else img.ctypes.data_as(u8p)

    def refused(word, *args):
        _arm(lib)
        fn(*args)
        msg = lib.stm_last_error()
        assert b"\n" + name[4:].encode() + b":" in msg and word in msg, (args[2:], msg)
        assert (out == 77).all()
    good = (rows, cols, E, 1.5, 0.0, 0.0)

    def with_arg(k, v):
        return good[:k] + (v,) + good[k + 1:]
    refused(b"num_rows", po, pi, *with_arg(0, 0))
    refused(b"num_cols", po, pi, *with_arg(1, 0))
    refused(b"elem_sz", po, pi, *with_arg(2, 2))
    for k in (3, 4, 5):
        for bad in (NAN, INF):
            refused(b"finite", po, pi, *with_arg(k, bad))
    refused(b"null", None, pi, *good)
    refused(b"null", po, None, *good)
    refused(b"overlap", pi, pi, *good)


@pytest.mark.parametrize("name", ["stm_align_fit", "stm_d_align_fit"])
def test_align_fit_rules(lib, name):
    fn = getattr(lib, name)
    rows, cols, E = 4, 8, 3
    img = np.zeros((rows, cols, E), np.uint8)
    state = np.full(4, 7.0, np.float32)
    dev = name == "stm_d_align_fit"
    pi = img.ctypes.data if dev else img.ctypes.data_as(u8p)
    ps = state.ctypes.data if dev else state.ctypes.data_as(f32p)
    tail = (None, None, None) if dev else ()

    def refused(word, l, r, st, *args):
        _arm(lib)
        res = fn(l, r, *args, st, *tail)
        msg = lib.stm_last_error()
        assert b"\n" + name[4:].encode() + b":" in msg and word in msg, (args, msg)
        assert dev or res == -1
        assert (state == 7.0).all()
    good = (rows, cols, E, 16, 1.0)

    def with_arg(k, v):
        return good[:k] + (v,) + good[k + 1:]
    refused(b"num_rows", pi, pi, ps, *with_arg(0, 3))
    refused(b"num_cols", pi, pi, ps, *with_arg(1, 7))
    refused(b"num_rows", pi, pi, ps, *with_arg(0, 0))
    refused(b"elem_sz", pi, pi, ps, *with_arg(2, 2))
    refused(b"radius", pi, pi, ps, *with_arg(3, 0))
    refused(b"radius", pi, pi, ps, *with_arg(3, 33))
    refused(b"rate", pi, pi, ps, *with_arg(4, 0.0))
    refused(b"rate", pi, pi, ps, *with_arg(4, NAN))
    refused(b"8421504", pi, pi, ps, 70000, 70000, E, 16, 1.0)  # sums that would not fit 32 bits
    refused(b"null", None, pi, ps, *good)
    refused(b"null", pi, None, ps, *good)
    refused(b"null", pi, pi, None, *good)
