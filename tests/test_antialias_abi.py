"""CPU checks of view antialiasing's C boundary (stm_set_antialias, stm_get_antialias, stm_view_prefilter / stm_d_view_prefilter,
stm_stream_set_antialias): declared, exported, prototyped with the right int / float / pointer kinds, usable from plain C and C++,
and the argument rules -- every refusal happens before anything is launched, so these run without a GPU.  (A frame stream cannot be
created without one: stm_stream_set_antialias's rules are in test_gpu_antialias.py.)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "include")
SYMBOLS = ["stm_set_antialias", "stm_get_antialias", "stm_view_prefilter", "stm_d_view_prefilter", "stm_stream_set_antialias"]
u8p = ctypes.POINTER(ctypes.c_uint8)
f32p = ctypes.POINTER(ctypes.c_float)
INF, NAN = float("inf"), float("nan")


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
    # (img_out, img, disp, num_rows, num_cols, elem_sz, num_views, float strength, max_radius, float gate, float gain, float conv)
    assert "".join(ctype_kind.get(a, "p") for a in _lib.PROTOS["stm_d_view_prefilter"][0]) == "pppiiiififff"
    assert "".join(ctype_kind.get(a, "p") for a in _lib.PROTOS["stm_set_antialias"][0]) == "ifif"


def test_calls_compile_from_plain_c_and_cxx(tmp_path):
    body = ('#include "stm_hip.h"\n'
            'int use(void *s, unsigned char *out, const unsigned char *img, const float *disp) {\n'
            '    int now[2];\n'
            '    float par[2];\n'
            '    if (stm_set_antialias(1, 1.0f, 8, 1.0f) != 0) return -1;\n'
            '    stm_get_antialias(now, par);\n'
            '    stm_view_prefilter(out, img, disp, 1080, 1920, 3, 8, par[0], now[1], par[1], 1.0f, 0.0f);\n'
            '    stm_d_view_prefilter(out, img, disp, 1080, 1920, 4, 48, 2.0f, 16, 0.5f, 0.8f, -3.0f);\n'
            '    return stm_stream_set_antialias(s, 1, 1.0f, 8, 1.0f) + stm_set_antialias(0, 0.0f, 0, 0.0f);\n'
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
        lib.stm_set_antialias(0, 0.0, 0, 0.0)
        lib.stm_set_error_mode(0)


def _arm(lib):
    """plant a known message: a later check sees the call's own message or this one, never an earlier call's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


def _setting(lib):
    m = (ctypes.c_int * 2)(-1, -1)
    v = (ctypes.c_float * 2)(-1.0, -1.0)
    lib.stm_get_antialias(m, ctypes.cast(v, f32p))
    return m[0], v[0], m[1], v[1]


# (strength, max_radius, gate) that every entry refuses, and the word the message must carry
PARAM_RULES = [((-0.5, 8, 1.0), b"strength"), ((8.5, 8, 1.0), b"strength"), ((NAN, 8, 1.0), b"strength"), ((INF, 8, 1.0), b"strength"),
               ((1.0, 0, 1.0), b"max_radius"), ((1.0, 17, 1.0), b"max_radius"), ((1.0, -3, 1.0), b"max_radius"),
               ((1.0, 8, -0.25), b"gate"), ((1.0, 8, NAN), b"gate"), ((1.0, 8, INF), b"gate")]


def test_get_antialias_defaults(lib):
    assert _setting(lib) == (0, 0.0, 0, 0.0)


def test_set_antialias_rules_leave_the_setting_unchanged(lib):
    assert lib.stm_set_antialias(1, 1.5, 6, 0.75) == 0
    assert _setting(lib) == (1, 1.5, 6, 0.75)
    for (args, word) in PARAM_RULES:
        _arm(lib)
        assert lib.stm_set_antialias(1, *args) == -1, args
        msg = lib.stm_last_error()
        assert b"\nset_antialias:" in msg and word in msg, (args, msg)
        assert _setting(lib) == (1, 1.5, 6, 0.75)
    for mode in (-1, 2, 7):
        _arm(lib)
        assert lib.stm_set_antialias(mode, 1.0, 8, 1.0) == -1
        assert b"mode" in lib.stm_last_error()
        assert _setting(lib) == (1, 1.5, 6, 0.75)
    # the edges of every range are accepted
    for args in ((0.0, 1, 0.0), (8.0, 16, 3.0e38)):
        assert lib.stm_set_antialias(1, *args) == 0, args
        assert _setting(lib) == (1,) + tuple(np.float32(a) if isinstance(a, float) else a for a in args)
    # mode 0 ignores the other arguments and reads back as the default
    assert lib.stm_set_antialias(0, NAN, -5, -1.0) == 0
    assert _setting(lib) == (0, 0.0, 0, 0.0)


def test_python_setter_raises_and_reads_back(lib):
    from stm_amd import device_api as dev
    dev.set_antialias(1, 2.0, 4, 0.5)
    assert dev.get_antialias() == (1, 2.0, 4, 0.5)
    with pytest.raises(ValueError, match="max_radius"):
        dev.set_antialias(1, 2.0, 40, 0.5)
    assert dev.get_antialias() == (1, 2.0, 4, 0.5)
    dev.set_antialias(0)
    assert dev.get_antialias() == (0, 0.0, 0, 0.0)


@pytest.mark.parametrize("name", ["stm_view_prefilter", "stm_d_view_prefilter"])
def test_stage_call_rules(lib, name):
    """both flavours refuse before anything is launched or written: out keeps its bytes"""
    fn = getattr(lib, name)
    rows, cols, E = 2, 5, 3
    img = np.arange(rows * cols * E, dtype=np.uint8).reshape(rows, cols, E)
    disp = np.zeros((rows, cols), np.float32)
    out = np.full((rows, cols, E), 77, np.uint8)
    dev = name == "stm_d_view_prefilter"
    po = out.ctypes.data if dev else out.ctypes.data_as(u8p)
    pi = img.ctypes.data if dev else img.ctypes.data_as(u8p)
    pd = disp.ctypes.data if dev else disp.ctypes.data_as(f32p)

    def refused(word, *args):
        _arm(lib)
        fn(*args)
        msg = lib.stm_last_error()
        assert b"\n" + name[4:].encode() + b":" in msg and word in msg, (args[3:], msg)
        assert (out == 77).all()
    good = (rows, cols, E, 8, 1.0, 8, 1.0, 1.0, 0.0)

    def with_arg(k, v):
        return good[:k] + (v,) + good[k + 1:]
    refused(b"num_rows", po, pi, pd, *with_arg(0, 0))
    refused(b"num_cols", po, pi, pd, *with_arg(1, 0))
    refused(b"elem_sz", po, pi, pd, *with_arg(2, 2))
    refused(b"num_views", po, pi, pd, *with_arg(3, 1))
    for ((s, r, g), word) in PARAM_RULES:
        refused(word, po, pi, pd, rows, cols, E, 8, s, r, g, 1.0, 0.0)
    for gain in (-0.5, 8.5, NAN):  # stm_set_depth's mode-1 rules
        refused(b"gain", po, pi, pd, *with_arg(7, gain))
    for conv in (4097.0, -INF, NAN):
        refused(b"conv", po, pi, pd, *with_arg(8, conv))
    refused(b"null", None, pi, pd, *good)
    refused(b"null", po, None, pd, *good)
    refused(b"null", po, pi, None, *good)
    # img_out must not overlap img: the same buffer, and one shifted by a pixel
    refused(b"overlap", pi, pi, pd, *good)
    buf = np.zeros(rows * cols * E + E, np.uint8)
    a, b = buf[:-E], buf[E:]
    refused(b"overlap", a.ctypes.data if dev else a.ctypes.data_as(u8p), b.ctypes.data if dev else b.ctypes.data_as(u8p), pd, *good)
