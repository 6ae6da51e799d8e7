"""CPU checks of the shot-change detector's C boundary (stm_set_cut, stm_get_cut, the two stage calls and the two frame-stream calls):
declared, exported, prototyped, usable from plain C and C++, the Python signatures, and the argument screening of every call that
screens before it touches the device (no compute calls -- there is no GPU here)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "include")
SYMBOLS = ["stm_set_cut", "stm_get_cut", "stm_cut_detect", "stm_d_cut_detect", "stm_stream_set_cut", "stm_stream_cut"]
u8p, i32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int)


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
            'int use(void *s, const unsigned char *l, int *st, float *depth, float *align, int *balance, unsigned int *sig) {\n'
            '    int m[3];\n'
            '    if (stm_set_cut(1, 370, 1, st) != 0) return -1;\n'
            '    stm_get_cut(m);\n'
            '    if (stm_set_cut(0, 0, 0, 0) != 0) return -1;\n'
            '    if (stm_cut_detect(l, 4, 8, 3, 370, 1, st) < 0) return -1;\n'
            '    stm_d_cut_detect(l, 4, 8, 3, 370, 1, st, depth, align, balance, sig);\n'
            '    stm_d_cut_detect(l, 4, 8, 3, 370, 1, st, 0, 0, 0, 0);\n'
            '    if (stm_stream_set_cut(s, 1, 370, 3) != 0) return -1;\n'
            '    return stm_stream_cut(s, m);\n'
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


def test_python_signatures(stm):
    from stm_amd import device_api as dev, host_api as host, video

    def names(f):
        return list(inspect.signature(f).parameters)
    assert names(dev.set_cut) == ["mode", "thresh_permille", "min_gap", "state"]
    assert names(dev.get_cut) == []
    assert names(dev.d_cut_detect) == ["img_l", "thresh_permille", "min_gap", "state", "resets", "sig"]
    assert names(host.cut_detect) == ["img_l", "thresh_permille", "min_gap", "state"]
    assert "cut" in names(video.FrameStream.__init__) and inspect.signature(video.FrameStream.__init__).parameters["cut"].default is None
    assert names(video.FrameStream.set_cut) == ["self", "mode", "thresh_permille", "min_gap"]
    assert names(video.FrameStream.cut) == ["self"]
    assert {"cut", "on_cut"} <= set(names(video.process_sequence))
    assert video.CUT_DEFAULT == (370, 3)
    assert inspect.signature(host.cut_detect).parameters["thresh_permille"].default == video.CUT_DEFAULT[0]
    assert inspect.signature(dev.set_cut).parameters["thresh_permille"].default == video.CUT_DEFAULT[0]
    assert inspect.signature(dev.set_cut).parameters["min_gap"].default == 1  # the C calls' default


def test_take_cut_option(stm):
    from stm_amd import video
    argv = ["x", "--cut", "a", "b"]
    assert video.take_cut_option(argv) == video.CUT_DEFAULT and argv == ["x", "a", "b"]
    argv = ["x", "--cut", "350", "5", "b"]
    assert video.take_cut_option(argv) == (350, 5) and argv == ["x", "b"]
    assert video.take_cut_option(["x", "y"]) is None
    for bad in (["--cut", "350"], ["--cut", "350", "x"], ["--cut", "0", "1"], ["--cut", "1001", "1"], ["--cut", "5", "0"],
                ["--cut", "5", str((1 << 20) + 1)]):
        with pytest.raises(ValueError):
            video.take_cut_option(list(bad))


@pytest.fixture
def lib(stm):
    lib = stm.lib()
    lib.stm_set_error_mode(1)
    try:
        yield lib
    finally:
        lib.stm_set_cut(0, 0, 0, None)
        lib.stm_set_error_mode(0)


def _arm(lib):
    """plant a known message: a later check sees the call's own message or this one, never an earlier call's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


def _setting(lib):
    m = (ctypes.c_int * 3)(-1, -1, -1)
    lib.stm_get_cut(m)
    return m[0], m[1], m[2]


def test_set_cut_rules_leave_the_setting_unchanged(lib):
    state = np.zeros(260, np.int32)  # never dereferenced by the setter
    ps = state.ctypes.data
    assert _setting(lib)[0] == 0
    assert lib.stm_set_cut(1, 1, 1, ps) == 0 and lib.stm_set_cut(1, 1000, 1 << 20, ps) == 0  # the edges are accepted
    assert lib.stm_set_cut(1, 420, 7, ps) == 0
    assert _setting(lib) == (1, 420, 7)
    for args, word in [((-1, 400, 1, ps), b"mode"), ((2, 400, 1, ps), b"mode"), ((1, 0, 1, ps), b"thresh_permille"),
                       ((1, 1001, 1, ps), b"thresh_permille"), ((1, -5, 1, ps), b"thresh_permille"), ((1, 400, 0, ps), b"min_gap"),
                       ((1, 400, (1 << 20) + 1, ps), b"min_gap"), ((1, 400, 1, None), b"d_state")]:
        _arm(lib)
        assert lib.stm_set_cut(*args) == -1, args
        msg = lib.stm_last_error()
        assert b"\nset_cut:" in msg and word in msg, msg
        assert _setting(lib) == (1, 420, 7)
    # mode 0 ignores the other arguments, whatever they are, and keeps the numbers
    assert lib.stm_set_cut(0, -9, -9, None) == 0
    assert _setting(lib) == (0, 420, 7)
    assert (state == 0).all()


def test_python_setter_raises_and_reads_back(lib):
    from stm_amd import device_api as dev
    with pytest.raises(ValueError, match="d_state"):
        dev.set_cut(1, 400, 2)
    with pytest.raises(ValueError, match="mode"):
        dev.set_cut(3)
    assert dev.get_cut()[0] == 0
    dev.set_cut(0)
    assert dev.get_cut()[0] == 0


@pytest.mark.parametrize("name", ["stm_cut_detect", "stm_d_cut_detect"])
def test_cut_detect_rules(lib, name):
    """both flavours refuse before anything is launched or written: the state keeps its words"""
    fn = getattr(lib, name)
    rows, cols, E = 4, 8, 3
    img = np.zeros((rows, cols, E), np.uint8)
    state = np.full(260, 7, np.int32)
    dev = name == "stm_d_cut_detect"
    pi = img.ctypes.data if dev else img.ctypes.data_as(u8p)
    ps = state.ctypes.data if dev else state.ctypes.data_as(i32p)
    tail = (None, None, None, None) if dev else ()

    def refused(word, l, st, *args):
        _arm(lib)
        res = fn(l, *args, st, *tail)
        msg = lib.stm_last_error()
        assert b"\n" + name[4:].encode() + b":" in msg and word in msg, (args, msg)
        assert dev or res == -1
        assert (state == 7).all()
    good = (rows, cols, E, 370, 1)

    def with_arg(k, v):
        return good[:k] + (v,) + good[k + 1:]
    refused(b"num_rows", pi, ps, *with_arg(0, 3))
    refused(b"num_rows", pi, ps, *with_arg(0, 0))
    refused(b"num_cols", pi, ps, *with_arg(1, 3))
    refused(b"num_cols", pi, ps, *with_arg(1, -8))
    refused(b"elem_sz", pi, ps, *with_arg(2, 2))
    refused(b"thresh_permille", pi, ps, *with_arg(3, 0))
    refused(b"thresh_permille", pi, ps, *with_arg(3, 1001))
    refused(b"min_gap", pi, ps, *with_arg(4, 0))
    refused(b"min_gap", pi, ps, *with_arg(4, (1 << 20) + 1))
    refused(b"2147483648", pi, ps, 65536, 32768, E, 370, 1)  # H * W = 2^31
    refused(b"2147483648", pi, ps, 70000, 70000, E, 370, 1)
    refused(b"null", None, ps, *good)
    refused(b"null", pi, None, *good)
