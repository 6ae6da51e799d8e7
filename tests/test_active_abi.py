"""CPU checks of the active picture area's C boundary (stm_set_active, stm_set_active_auto, stm_get_active, the eight stage calls and
the two frame-stream calls): declared, exported, prototyped, usable from plain C and C++, the Python signatures, the argument
screening of every call that screens before it touches the device, and the drivers' options (no compute calls -- there is no GPU
here)."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "include")
SYMBOLS = ["stm_set_active", "stm_set_active_auto", "stm_get_active", "stm_active_detect", "stm_d_active_detect", "stm_active_fill",
           "stm_d_active_fill", "stm_depth_fit_rect", "stm_d_depth_fit_rect", "stm_overlay_fit_rect", "stm_d_overlay_fit_rect",
           "stm_stream_set_active", "stm_stream_active"]
u8p, i32p, f32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)
DEFAULT = (0, 0, 0, 0, 0, 0, 24, 10, 300, 12, 0.0)


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
            'int use(void *s, const unsigned char *l, int *st, const int *cut, unsigned int *counts, float *d, float *fs) {\n'
            '    int m[10], r[4] = {1, 3, 0, 8}, o[5];\n'
            '    float v;\n'
            '    if (stm_set_active(1, r, 1, -2.5f) != 0) return -1;\n'
            '    if (stm_set_active_auto(24, 10, 300, 12, st) != 0) return -1;\n'
            '    stm_get_active(m, &v);\n'
            '    if (stm_set_active(0, 0, 0, 0.0f) != 0) return -1;\n'
            '    if (stm_active_detect(l, 4, 8, 3, 24, 10, 300, 12, 0, st) < 0) return -1;\n'
            '    stm_d_active_detect(l, 4, 8, 3, 24, 10, 300, 12, 1, st, cut, counts);\n'
            '    stm_d_active_detect(l, 4, 8, 3, 24, 10, 300, 12, 0, st, 0, 0);\n'
            '    stm_active_fill(d, 4, 8, r, 0.0f);\n'
            '    stm_d_active_fill(d, 4, 8, st + 1, 0.0f);\n'
            '    stm_depth_fit_rect(d, d, 4, 8, -4.0f, 4.0f, 1.0f, 20, 1.0f, fs, r);\n'
            '    stm_d_depth_fit_rect(d, d, 4, 8, -4.0f, 4.0f, 1.0f, 20, 1.0f, fs, st + 1);\n'
            '    stm_overlay_fit_rect(d, d, 4, 8, l, 1, 1, 0, 0, 4, 8, 1.0f, 0.0f, 20, 1.0f, 8, -8.0f, 8.0f, 1.0f, 0.1f, 0, fs, r);\n'
            '    stm_d_overlay_fit_rect(d, d, 4, 8, l, 1, 1, 0, 0, 4, 8, 1.0f, 0.0f, 20, 1.0f, 8, -8.0f, 8.0f, 1.0f, 0.1f, 0, fs, cut, st + 1);\n'
            '    if (stm_stream_set_active(s, 2, 0, 1, 0.0f, 24, 10, 300, 12) != 0) return -1;\n'
            '    return stm_stream_active(s, o);\n'
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
    assert names(dev.set_active) == ["mode", "rect", "fill", "fill_disp"]
    assert names(dev.set_active_auto) == ["thresh_luma", "lit_permille", "max_bar_permille", "hold", "state"]
    assert names(dev.get_active) == []
    assert names(dev.d_active_detect)[:2] == ["img_l", "state"] and {"restart", "cut_state", "counts"} <= set(names(dev.d_active_detect))
    assert names(dev.d_active_fill) == ["disp", "rect", "value"]
    assert names(dev.d_depth_fit_rect) == names(dev.d_depth_fit) + ["rect"]
    assert "rect" in names(dev.d_overlay_fit_rect) and set(names(dev.d_overlay_fit)) <= set(names(dev.d_overlay_fit_rect))
    assert names(host.active_detect) == ["img_l", "thresh_luma", "lit_permille", "max_bar_permille", "hold", "restart", "state"]
    assert names(host.active_fill) == ["disp", "rect", "value"]
    assert names(host.depth_fit_rect) == names(host.depth_fit) + ["rect"]
    assert names(host.overlay_fit_rect) == names(host.overlay_fit) + ["rect"]
    init = inspect.signature(video.FrameStream.__init__).parameters
    for k in ("active", "active_auto", "active_fill"):
        assert k in init and init[k].default is None
    assert names(video.FrameStream.active) == ["self"]
    assert {"active", "active_auto", "active_fill", "on_active"} <= set(names(video.process_sequence))
    assert video.ACTIVE_AUTO_DEFAULT == (24, 10, 300, 12) == dev.ACTIVE_AUTO_DEFAULTS
    sig = inspect.signature(dev.set_active_auto).parameters
    assert tuple(sig[k].default for k in ("thresh_luma", "lit_permille", "max_bar_permille", "hold")) == video.ACTIVE_AUTO_DEFAULT


def test_take_active_options(stm):
    from stm_amd import video
    argv = ["x", "--active", "49", "335", "0", "640", "b"]
    assert video.take_active_options(argv) == ((49, 335, 0, 640), None, None) and argv == ["x", "b"]
    argv = ["x", "--active-auto", "a", "--active-fill", "-2.5"]
    assert video.take_active_options(argv) == (None, video.ACTIVE_AUTO_DEFAULT, -2.5) and argv == ["x", "a"]
    argv = ["x", "--active-auto", "32", "5", "450", "1", "b"]
    assert video.take_active_options(argv) == (None, (32, 5, 450, 1), None) and argv == ["x", "b"]
    assert video.take_active_options(["x", "y"]) == (None, None, None)
    for bad in (["--active", "1", "2", "3"], ["--active", "1", "2", "3", "x"], ["--active", "5", "5", "0", "8"], ["--active", "-1", "5", "0", "8"],
                ["--active", "0", "5", "8", "8"], ["--active-auto", "24"], ["--active-auto", "24", "10", "300"], ["--active-auto", "255", "10", "300", "12"],
                ["--active-auto", "24", "1000", "300", "12"], ["--active-auto", "24", "10", "451", "12"], ["--active-auto", "24", "10", "300", "0"],
                ["--active-auto", "24", "10", "300", str((1 << 20) + 1)], ["--active-fill", "0"], ["--active-auto", "--active-fill"],
                ["--active-auto", "--active-fill", "x"], ["--active-auto", "--active-fill", "5000"], ["--active-auto", "--active-fill", "nan"],
                ["--active", "0", "5", "0", "8", "--active-auto"]):
        with pytest.raises(ValueError):
            video.take_active_options(list(bad))


@pytest.mark.parametrize("tool,nargs", [("stm_video", 16), ("stm_image", 17)])
def test_the_drivers_refuse_malformed_options(capsys, tool, nargs):
    """usage and -1, before any frame is read"""
    spec = importlib.util.spec_from_file_location(tool, os.path.join(ROOT, "tools", tool + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for tail in (["--active", "1", "2", "3"], ["--active", "5", "5", "0", "8"], ["--active-auto", "24", "10"], ["--active-auto", "24", "10", "300", "0"],
                 ["--active-fill", "1"], ["--active-auto", "--active-fill", "x"], ["--active", "0", "5", "0", "8", "--active-auto"]):
        assert mod.main([tool] + ["x"] * (nargs - 1) + tail) == -1, tail
        assert "--active T B L R | --active-auto [THRESH LIT MAX_BAR HOLD]" in capsys.readouterr().out


@pytest.fixture
def lib(stm):
    lib = stm.lib()
    lib.stm_set_error_mode(1)
    try:
        yield lib
    finally:
        lib.stm_set_active(0, None, 0, 0.0)
        lib.stm_set_active_auto(24, 10, 300, 12, None)
        lib.stm_set_error_mode(0)


def _arm(lib):
    """plant a known message: a later check sees the call's own message or this one, never an earlier call's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


def _setting(lib):
    m = (ctypes.c_int * 10)(*([-1] * 10))
    v = ctypes.c_float(-1.0)
    lib.stm_get_active(m, ctypes.cast(ctypes.byref(v), f32p))
    return tuple(m) + (float(v.value),)


def _rect(*v):
    return (ctypes.c_int * 4)(*v)


def test_the_getters_defaults(lib):
    assert _setting(lib) == DEFAULT
    from stm_amd import device_api as dev
    assert dev.get_active() == (0, (0, 0, 0, 0), 0, 0.0, 24, 10, 300, 12)


def test_set_active_rules_leave_the_setting_unchanged(lib):
    assert lib.stm_set_active(1, _rect(0, 1, 0, 1), 0, 4096.0) == 0 and lib.stm_set_active(2, None, 1, -4096.0) == 0  # the edges
    assert lib.stm_set_active(1, _rect(49, 335, 0, 640), 1, -2.5) == 0
    kept = (1, 49, 335, 0, 640, 1, 24, 10, 300, 12, -2.5)
    assert _setting(lib) == kept
    r = _rect(1, 5, 2, 6)
    for args, word in [((-1, r, 0, 0.0), b"mode"), ((3, r, 0, 0.0), b"mode"), ((1, None, 0, 0.0), b"rect"), ((1, _rect(-1, 5, 2, 6), 0, 0.0), b"rect"),
                       ((1, _rect(5, 5, 2, 6), 0, 0.0), b"rect"), ((1, _rect(6, 5, 2, 6), 0, 0.0), b"rect"), ((1, _rect(1, 5, -2, 6), 0, 0.0), b"rect"),
                       ((1, _rect(1, 5, 6, 6), 0, 0.0), b"rect"), ((1, r, 2, 0.0), b"fill"), ((1, r, -1, 0.0), b"fill"), ((2, None, 2, 0.0), b"fill"),
                       ((1, r, 1, 4097.0), b"fill_disp"), ((2, None, 0, float("nan")), b"fill_disp"), ((2, None, 1, float("inf")), b"fill_disp")]:
        _arm(lib)
        assert lib.stm_set_active(*args) == -1, args
        msg = lib.stm_last_error()
        assert b"\nset_active:" in msg and word in msg, msg
        assert _setting(lib) == kept
    # mode 0 ignores the other arguments, whatever they are, and keeps mode 2's numbers
    assert lib.stm_set_active_auto(30, 5, 450, 1, None) == 0
    assert lib.stm_set_active(0, None, 7, float("nan")) == 0
    assert _setting(lib) == (0, 0, 0, 0, 0, 0, 30, 5, 450, 1, 0.0)


def test_set_active_auto_rules_leave_the_parameters_unchanged(lib):
    state = np.zeros(16, np.int32)  # never dereferenced by the setter
    ps = state.ctypes.data
    assert lib.stm_set_active_auto(0, 0, 0, 1, ps) == 0 and lib.stm_set_active_auto(254, 999, 450, 1 << 20, None) == 0  # the edges
    assert lib.stm_set_active_auto(32, 7, 250, 6, ps) == 0
    assert _setting(lib)[6:10] == (32, 7, 250, 6)
    for args, word in [((-1, 7, 250, 6), b"thresh_luma"), ((255, 7, 250, 6), b"thresh_luma"), ((32, -1, 250, 6), b"lit_permille"),
                       ((32, 1000, 250, 6), b"lit_permille"), ((32, 7, -1, 6), b"max_bar_permille"), ((32, 7, 451, 6), b"max_bar_permille"),
                       ((32, 7, 250, 0), b"hold"), ((32, 7, 250, (1 << 20) + 1), b"hold")]:
        _arm(lib)
        assert lib.stm_set_active_auto(*args, ps) == -1, args
        msg = lib.stm_last_error()
        assert b"\nset_active_auto:" in msg and word in msg, msg
        assert _setting(lib)[6:10] == (32, 7, 250, 6)
    # kept when the mode changes
    assert lib.stm_set_active(2, None, 0, 0.0) == 0 and lib.stm_set_active(0, None, 0, 0.0) == 0
    assert _setting(lib)[6:10] == (32, 7, 250, 6)
    assert (state == 0).all()


def test_python_setters_raise_and_read_back(lib):
    from stm_amd import device_api as dev
    with pytest.raises(ValueError, match="rect"):
        dev.set_active(1)
    with pytest.raises(ValueError, match="mode"):
        dev.set_active(3)
    with pytest.raises(ValueError, match="hold"):
        dev.set_active_auto(hold=0)
    dev.set_active(1, (2, 9, 1, 7), fill=True, fill_disp=1.5)
    assert dev.get_active() == (1, (2, 9, 1, 7), 1, 1.5, 24, 10, 300, 12)
    dev.set_active(0)
    assert dev.get_active()[0] == 0


@pytest.mark.parametrize("name", ["stm_active_detect", "stm_d_active_detect"])
def test_active_detect_rules(lib, name):
    """both flavours refuse before anything is launched or written: the state keeps its words"""
    fn = getattr(lib, name)
    rows, cols, E = 4, 8, 3
    img = np.zeros((rows, cols, E), np.uint8)
    state = np.full(16, 7, np.int32)
    dev = name == "stm_d_active_detect"
    pi = img.ctypes.data if dev else img.ctypes.data_as(u8p)
    ps = state.ctypes.data if dev else state.ctypes.data_as(i32p)
    tail = (None, None) if dev else ()

    def refused(word, l, st, *args):
        _arm(lib)
        res = fn(l, *args, st, *tail)
        msg = lib.stm_last_error()
        assert b"\n" + name[4:].encode() + b":" in msg and word in msg, (args, msg)
        assert dev or res == -1
        assert (state == 7).all()
    good = (rows, cols, E, 24, 10, 300, 12, 0)

    def with_arg(k, v):
        return good[:k] + (v,) + good[k + 1:]
    refused(b"num_rows", pi, ps, *with_arg(0, 0))
    refused(b"num_cols", pi, ps, *with_arg(1, -8))
    refused(b"elem_sz", pi, ps, *with_arg(2, 2))
    refused(b"thresh_luma", pi, ps, *with_arg(3, -1))
    refused(b"thresh_luma", pi, ps, *with_arg(3, 255))
    refused(b"lit_permille", pi, ps, *with_arg(4, 1000))
    refused(b"max_bar_permille", pi, ps, *with_arg(5, 451))
    refused(b"hold", pi, ps, *with_arg(6, 0))
    refused(b"hold", pi, ps, *with_arg(6, (1 << 20) + 1))
    refused(b"2147483648", pi, ps, 65536, 32768, E, 24, 10, 300, 12, 0)  # H * W = 2^31
    refused(b"null", None, ps, *good)
    refused(b"null", pi, None, *good)


def test_fill_and_fit_rect_rules(lib):
    """the host flavours screen their four ints against the map before anything is launched or written"""
    d = np.full((4, 8), 3.0, np.float32)
    pd = d.ctypes.data_as(f32p)
    st = np.full(4, 9.0, np.float32)
    pst = st.ctypes.data_as(f32p)
    ov = np.full((1, 1, 4), 255, np.uint8)
    for bad in ((0, 5, 0, 8), (0, 4, 0, 9), (2, 2, 0, 8), (-1, 4, 0, 8), (0, 4, 3, 3)):
        r = _rect(*bad)
        _arm(lib)
        lib.stm_active_fill(pd, 4, 8, r, 0.0)
        msg = lib.stm_last_error()
        assert b"\nactive_fill:" in msg and b"rect" in msg, (bad, msg)
        _arm(lib)
        lib.stm_depth_fit_rect(pd, pd, 4, 8, -4.0, 4.0, 1.0, 20, 1.0, pst, r)
        msg = lib.stm_last_error()
        assert b"\ndepth_fit_rect:" in msg and b"rect" in msg, (bad, msg)
        _arm(lib)
        lib.stm_overlay_fit_rect(pd, pd, 4, 8, ov.ctypes.data_as(u8p), 1, 1, 0, 0, 4, 8, 1.0, 0.0, 20, 1.0, 8, -8.0, 8.0, 1.0, 0.1, 0, pst, r)
        msg = lib.stm_last_error()
        assert b"\noverlay_fit_rect:" in msg and b"rect" in msg, (bad, msg)
    for name, args in (("active_fill", (pd, 0, 8, _rect(0, 4, 0, 8), 0.0)), ("active_fill", (None, 4, 8, _rect(0, 4, 0, 8), 0.0)),
                       ("d_active_fill", (None, 4, 8, None, 0.0)), ("d_active_fill", (d.ctypes.data, 4, 0, None, 0.0))):
        _arm(lib)
        getattr(lib, "stm_" + name)(*args)
        assert b"\n" + name.encode() + b":" in lib.stm_last_error(), name
    # the other arguments keep stm_depth_fit's and stm_overlay_fit's rules
    _arm(lib)
    lib.stm_depth_fit_rect(pd, pd, 4, 8, 4.0, -4.0, 1.0, 20, 1.0, pst, None)
    assert b"\ndepth_fit_rect:" in lib.stm_last_error()
    _arm(lib)
    lib.stm_d_depth_fit_rect(d.ctypes.data, d.ctypes.data, 4, 8, -4.0, 4.0, 1.0, 500, 1.0, st.ctypes.data, None)
    assert b"\nd_depth_fit_rect:" in lib.stm_last_error()
    _arm(lib)
    lib.stm_d_overlay_fit_rect(d.ctypes.data, d.ctypes.data, 4, 8, ov.ctypes.data, 1, 1, 0, 0, 4, 8, 1.0, 0.0, 500, 1.0, 8, -8.0, 8.0, 1.0, 0.1, 0,
                               st.ctypes.data, None, None)
    assert b"\nd_overlay_fit_rect:" in lib.stm_last_error()
    assert (d == 3.0).all() and (st == 9.0).all()


FRAME = (64, 192, 96, 64, 96, 3, 8, 18.43, 16, 8, 10.0, 30.0, 6.0, 20.0, 17, 8, 20, 0.4)  # num_rows .. thresh_h of a 64 x 96 frame


@pytest.mark.parametrize("rect", [(0, 65, 0, 96), (0, 64, 0, 97), (10, 64, 90, 200)])
def test_a_mode_1_rectangle_that_does_not_fit_the_frame_is_refused_before_anything_is_launched(lib, rect):
    """the pointers are never dereferenced: the screen comes first, in the device flavours and through frame_host in the host ones"""
    assert lib.stm_set_active(1, _rect(*rect), 0, 0.0) == 0  # the setter knows no frame
    _arm(lib)
    lib.stm_d_adcensus_stm(None, None, None, None, *FRAME, 3)
    msg = lib.stm_last_error()
    assert b"\nd_adcensus_stm:" in msg and b"rect" in msg, msg
    _arm(lib)
    lib.stm_d_adcensus_stm_2s(None, None, None, None, *FRAME[:5], 32, 48, FRAME[5], 0.5, *FRAME[6:], 3)
    msg = lib.stm_last_error()
    assert b"\nd_adcensus_stm_2s:" in msg and b"rect" in msg, msg
    out = np.zeros((64, 96, 3), np.uint8)
    dl = np.full((64, 96), 5.0, np.float32)
    sbs = np.zeros((64, 192, 3), np.uint8)
    _arm(lib)
    lib.stm_adcensus_stm(sbs.ctypes.data_as(u8p), dl.ctypes.data_as(f32p), dl.ctypes.data_as(f32p), out.ctypes.data_as(u8p), *FRAME)
    msg = lib.stm_last_error()
    assert b"\nadcensus_stm:" in msg and b"rect" in msg, msg
    assert (dl == 5.0).all() and (out == 0).all()


def test_mode_2_refuses_a_frame_of_2_to_the_31_pixels(lib):
    assert lib.stm_set_active(2, None, 0, 0.0) == 0
    big = (65536, 65536, 32768) + FRAME[3:]
    _arm(lib)
    lib.stm_d_adcensus_stm(None, None, None, None, *big, 3)
    msg = lib.stm_last_error()
    assert b"\nd_adcensus_stm:" in msg and b"2147483648" in msg, msg
