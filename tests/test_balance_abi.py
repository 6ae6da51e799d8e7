"""CPU checks of the colour balance's C boundary (stm_set_balance, stm_set_balance_auto, stm_get_balance, the four stage calls and the
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
SYMBOLS = ["stm_set_balance", "stm_set_balance_auto", "stm_get_balance", "stm_balance_fit", "stm_d_balance_fit", "stm_balance_apply",
           "stm_d_balance_apply", "stm_stream_set_balance", "stm_stream_set_balance_auto", "stm_stream_balance"]
NAN, INF = float("nan"), float("inf")
u8p, i32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int)
IDENTITY = np.tile(np.arange(256, dtype=np.uint8), 3)


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
            'int use(void *s, unsigned char *o, const unsigned char *l, const unsigned char *r, int *st, unsigned int *w) {\n'
            '    int m[2]; float rate; unsigned char lut[768];\n'
            '    if (stm_set_balance_auto(48, 1.0f, st) != 0) return -1;\n'
            '    if (stm_set_balance(2, 0) != 0) return -1;\n'
            '    stm_get_balance(m, &rate, lut);\n'
            '    if (stm_set_balance(1, lut) != 0) return -1;\n'
            '    if (stm_balance_fit(l, r, 4, 8, 3, 48, 1.0f, st) < 0) return -1;\n'
            '    stm_d_balance_fit(l, r, 4, 8, 3, 48, 1.0f, st, w);\n'
            '    stm_balance_apply(o, l, 4, 8, 3, lut, 0);\n'
            '    stm_d_balance_apply(o, l, 4, 8, 3, 0, st);\n'
            '    if (stm_stream_set_balance_auto(s, 48, 0.25f) != 0) return -1;\n'
            '    if (stm_stream_set_balance(s, 2, 0) != 0) return -1;\n'
            '    return stm_stream_balance(s, lut);\n'
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
        lib.stm_set_balance_auto(48, 1.0, None)
        lib.stm_set_balance(0, None)
        lib.stm_set_error_mode(0)


def _arm(lib):
    """plant a known message: a later check sees the call's own message or this one, never an earlier call's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


def _setting(lib):
    m = (ctypes.c_int * 2)(-1, -1)
    r = ctypes.c_float(-1.0)
    t = (ctypes.c_uint8 * 768)()
    lib.stm_get_balance(m, ctypes.byref(r), t)
    return m[0], m[1], r.value, np.frombuffer(bytes(t), np.uint8)


def _same_setting(a, b):
    return a[:3] == b[:3] and np.array_equal(a[3], b[3])


def _lut(a):
    return (ctypes.c_uint8 * 768).from_buffer_copy(np.ascontiguousarray(a, np.uint8).tobytes())


def test_get_balance_defaults(lib):
    assert _same_setting(_setting(lib), (0, 48, 1.0, IDENTITY))


def test_set_balance_rules_leave_the_setting_unchanged(lib):
    table = np.random.RandomState(1).randint(0, 256, size=768).astype(np.uint8)
    buf = _lut(table)
    assert lib.stm_set_balance(1, buf) == 0
    buf[5] = (buf[5] + 1) & 255  # the table was copied: the caller's array is its own again
    assert _same_setting(_setting(lib), (1, 48, 1.0, table))
    for mode in (-1, 3, 9):
        _arm(lib)
        assert lib.stm_set_balance(mode, buf) == -1
        msg = lib.stm_last_error()
        assert b"\nset_balance:" in msg and b"mode" in msg, msg
        assert _same_setting(_setting(lib), (1, 48, 1.0, table))
    _arm(lib)
    assert lib.stm_set_balance(1, None) == -1
    msg = lib.stm_last_error()
    assert b"\nset_balance:" in msg and b"lut768" in msg and b"null" in msg, msg
    assert _same_setting(_setting(lib), (1, 48, 1.0, table))
    # modes 0 and 2 ignore the table and read back the identity; the automatic parameters are kept across the modes
    assert lib.stm_set_balance_auto(7, 0.5, None) == 0
    assert lib.stm_set_balance(2, None) == 0
    assert _same_setting(_setting(lib), (2, 7, 0.5, IDENTITY))
    assert lib.stm_set_balance(2, buf) == 0
    assert _same_setting(_setting(lib), (2, 7, 0.5, IDENTITY))
    assert lib.stm_set_balance(0, None) == 0
    assert _same_setting(_setting(lib), (0, 7, 0.5, IDENTITY))


def test_set_balance_auto_rules(lib):
    assert lib.stm_set_balance_auto(0, 1.0, None) == 0 and lib.stm_set_balance_auto(255, 1.0e-6, None) == 0  # the edges are accepted
    assert lib.stm_set_balance_auto(9, 0.25, None) == 0
    for (shift, rate), word in [((-1, 0.5), b"max_shift"), ((256, 0.5), b"max_shift"), ((1000, 0.5), b"max_shift"), ((8, 0.0), b"rate"),
                                ((8, 1.5), b"rate"), ((8, -0.5), b"rate"), ((8, NAN), b"rate"), ((8, INF), b"rate")]:
        _arm(lib)
        assert lib.stm_set_balance_auto(shift, rate, None) == -1, (shift, rate)
        msg = lib.stm_last_error()
        assert b"\nset_balance_auto:" in msg and word in msg, msg
        assert _setting(lib)[1:3] == (9, 0.25)


def test_python_setters_raise_and_read_back(lib):
    from stm_amd import device_api as dev
    table = np.arange(768).astype(np.uint8).reshape(3, 256)[:, ::-1]
    dev.set_balance_auto(12, 0.5)
    dev.set_balance(1, table)
    mode, shift, rate, lut = dev.get_balance()
    assert (mode, shift, rate) == (1, 12, 0.5) and lut.shape == (3, 256) and np.array_equal(lut, table)
    with pytest.raises(ValueError, match="lut768"):
        dev.set_balance(1)
    with pytest.raises(ValueError, match="768"):
        dev.set_balance(1, np.zeros(700, np.uint8))
    with pytest.raises(ValueError, match="max_shift"):
        dev.set_balance_auto(300, 0.5)
    with pytest.raises(ValueError, match="rate"):
        dev.set_balance_auto(30, NAN)
    assert dev.get_balance()[:3] == (1, 12, 0.5) and np.array_equal(dev.get_balance()[3], table)
    dev.set_balance(0)
    assert dev.get_balance()[0] == 0


@pytest.mark.parametrize("name", ["stm_balance_apply", "stm_d_balance_apply"])
def test_balance_apply_rules(lib, name):
    """both flavours refuse before anything is launched or written: out keeps its bytes"""
    fn = getattr(lib, name)
    rows, cols, E = 2, 5, 3
    img = np.arange(rows * cols * E, dtype=np.uint8).reshape(rows, cols, E)
    out = np.full((rows, cols, E), 77, np.uint8)
    state = np.zeros(769, np.int32)
    dev = name == "stm_d_balance_apply"
    po = out.ctypes.data if dev else out.ctypes.data_as(u8p)
    pi = img.ctypes.data if dev else img.ctypes.data_as(u8p)
    ps = state.ctypes.data if dev else state.ctypes.data_as(i32p)
    lut = _lut(IDENTITY)

    def refused(word, o, i, r, c, e, l, s):
        _arm(lib)
        fn(o, i, r, c, e, l, s)
        msg = lib.stm_last_error()
        assert b"\n" + name[4:].encode() + b":" in msg and word in msg, ((r, c, e), msg)
        assert (out == 77).all()
    refused(b"num_rows", po, pi, 0, cols, E, lut, None)
    refused(b"num_rows", po, pi, -3, cols, E, lut, None)
    refused(b"num_cols", po, pi, rows, 0, E, lut, None)
    refused(b"elem_sz", po, pi, rows, cols, 2, lut, None)
    refused(b"null", None, pi, rows, cols, E, lut, None)
    refused(b"null", po, None, rows, cols, E, lut, None)
    refused(b"exactly one", po, pi, rows, cols, E, None, None)  # neither
    refused(b"exactly one", po, pi, rows, cols, E, lut, ps)     # both
    refused(b"overlap", pi, pi, rows, cols, E, lut, None)


@pytest.mark.parametrize("name", ["stm_balance_fit", "stm_d_balance_fit"])
def test_balance_fit_rules(lib, name):
    fn = getattr(lib, name)
    rows, cols, E = 4, 8, 3
    img = np.zeros((rows, cols, E), np.uint8)
    state = np.full(769, 7, np.int32)
    dev = name == "stm_d_balance_fit"
    pi = img.ctypes.data if dev else img.ctypes.data_as(u8p)
    ps = state.ctypes.data if dev else state.ctypes.data_as(i32p)
    tail = (None,) if dev else ()

    def refused(word, l, r, st, *args):
        _arm(lib)
        res = fn(l, r, *args, st, *tail)
        msg = lib.stm_last_error()
        assert b"\n" + name[4:].encode() + b":" in msg and word in msg, (args, msg)
        assert dev or res == -1
        assert (state == 7).all()
    good = (rows, cols, E, 48, 1.0)

    def with_arg(k, v):
        return good[:k] + (v,) + good[k + 1:]
    refused(b"num_rows", pi, pi, ps, *with_arg(0, 0))
    refused(b"num_cols", pi, pi, ps, *with_arg(1, 0))
    refused(b"num_cols", pi, pi, ps, *with_arg(1, -8))
    refused(b"elem_sz", pi, pi, ps, *with_arg(2, 2))
    refused(b"max_shift", pi, pi, ps, *with_arg(3, -1))
    refused(b"max_shift", pi, pi, ps, *with_arg(3, 256))
    refused(b"rate", pi, pi, ps, *with_arg(4, 0.0))
    refused(b"rate", pi, pi, ps, *with_arg(4, 1.25))
    refused(b"rate", pi, pi, ps, *with_arg(4, NAN))
    refused(b"2147483648", pi, pi, ps, 65536, 32768, E, 48, 1.0)  # H * W = 2^31
    refused(b"2147483648", pi, pi, ps, 70000, 70000, E, 48, 1.0)
    refused(b"null", None, pi, ps, *good)
    refused(b"null", pi, None, ps, *good)
    refused(b"null", pi, pi, None, *good)


def test_rate_q_matches_the_statement():
    """the host's rate_q is the statement's (checked through the numbers of the definition, no GPU)"""
    from test_balance_ref import rate_q_ref
    assert [rate_q_ref(r) for r in (1.0, 0.5, 1.0 / 256, 1.0 / 1024, 0.75)] == [256, 128, 1, 1, 192]
