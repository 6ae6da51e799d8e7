"""CPU checks of the overlay's C boundary (stm_set_overlay, stm_get_overlay, stm_mux_overlay / stm_d_mux_overlay,
stm_stream_set_overlay, stm_stream_overlay): declared, exported, prototyped with the right int / float / double / pointer kinds, usable
from plain C and C++, and the argument rules -- every refusal happens before anything is launched, so these run without a GPU.  (A
frame stream cannot be created without one: the two stream calls' rules are in test_gpu_overlay.py.)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "include")
SYMBOLS = ["stm_set_overlay", "stm_get_overlay", "stm_mux_overlay", "stm_d_mux_overlay", "stm_stream_set_overlay", "stm_stream_overlay"]
u8p = ctypes.POINTER(ctypes.c_uint8)
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
    """argument count and the int / float / double / pointer kind of every argument, read off the header"""
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
    # (frame, overlay, ov_rows, ov_cols, x0, y0, float disparity, num_views, float angle, lens_mode, double pitch, slope, centre, ...)
    assert "".join(ctype_kind.get(a, "p") for a in _lib.PROTOS["stm_d_mux_overlay"][0]) == "ppiiiififidddiiiiiii"


def test_calls_compile_from_plain_c_and_cxx(tmp_path):
    body = ('#include "stm_hip.h"\n'
            'int use(void *s, unsigned char *frame, const unsigned char *ov) {\n'
            '    int now[5];\n'
            '    float disparity;\n'
            '    if (stm_set_overlay(1, ov, 120, 1920, 0, 900, -8.0f) != 0) return -1;\n'
            '    stm_get_overlay(now, &disparity);\n'
            '    stm_mux_overlay(frame, ov, now[1], now[2], now[3], now[4], disparity, 8, 18.43f, 0, 0.0, 0.0, 0.0, 0, 1, 1, 0, 1080, 1920, 3);\n'
            '    stm_d_mux_overlay(frame, ov, 420, 560, 0, 0, 2.5f, 48, 0.0f, 0, 0.0, 0.0, 0.0, 1, 8, 6, 3, 3360, 3360, 4);\n'
            '    stm_d_mux_overlay(frame, ov, 1, 1, -3, 7, 0.0f, 8, 0.0f, 3, 7.37, 0.86, 0.3, 0, 1, 1, 0, 1080, 1920, 3);\n'
            '    if (stm_stream_set_overlay(s, 120, 1920) != 0) return -1;\n'
            '    return stm_stream_overlay(s, ov, 120, 1920, 0, 900, -8.0f) + stm_set_overlay(0, 0, 0, 0, 0, 0, 0.0f);\n'
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
        lib.stm_set_overlay(0, None, 0, 0, 0, 0, 0.0)
        lib.stm_set_output(0, 0, 0, 0)
        lib.stm_set_layout(0, 0, 0, 0, 0)
        lib.stm_set_lens(0, 0.0, 0.0, 0.0)
        lib.stm_set_error_mode(0)


def _arm(lib):
    """plant a known message: a later check sees the call's own message or this one, never an earlier call's"""
    lib.stm_d_filter_median(None, 0, 0)
    assert b"d_filter_median" in lib.stm_last_error()


def _overlay(lib):
    now = (ctypes.c_int * 5)()
    disp = ctypes.c_float(-1.0)
    lib.stm_get_overlay(now, ctypes.byref(disp))
    return tuple(now) + (disp.value,)


# the overlay's own arguments (ov_rows, ov_cols, x0, y0, disparity) that every entry refuses, and the word the message must carry
OVERLAY_RULES = [((0, 5, 0, 0, 0.0), b"ov_rows"), ((65536, 5, 0, 0, 0.0), b"ov_rows"), ((-1, 5, 0, 0, 0.0), b"ov_rows"),
                 ((3, 0, 0, 0, 0.0), b"ov_cols"), ((3, 65536, 0, 0, 0.0), b"ov_cols"), ((3, 5, 65537, 0, 0.0), b"x0"),
                 ((3, 5, -65537, 0, 0.0), b"x0"), ((3, 5, 0, 65537, 0.0), b"y0"), ((3, 5, 0, -65537, 0.0), b"y0"),
                 ((3, 5, 0, 0, INF), b"disparity"), ((3, 5, 0, 0, -INF), b"disparity"), ((3, 5, 0, 0, NAN), b"disparity"),
                 ((3, 5, 0, 0, 4096.5), b"disparity"), ((3, 5, 0, 0, -4097.0), b"disparity")]


def test_set_overlay_rules_leave_the_state_readable(lib):
    assert _overlay(lib) == (0, 0, 0, 0, 0, 0.0)  # the default
    ov = np.zeros((3, 5, 4), np.uint8)  # (host memory stands in for the device pointer: the setter only records it)
    assert ov.ctypes.data % 4 == 0
    assert lib.stm_set_overlay(1, ov.ctypes.data, 3, 5, -2, 7, -13.75) == 0
    assert _overlay(lib) == (1, 3, 5, -2, 7, -13.75)
    refusals = [((2, ov.ctypes.data, 3, 5, 0, 0, 0.0), b"mode"), ((-1, ov.ctypes.data, 3, 5, 0, 0, 0.0), b"mode"),
                ((1, None, 3, 5, 0, 0, 0.0), b"null"), ((1, ov.ctypes.data + 1, 3, 5, 0, 0, 0.0), b"aligned"),
                ((1, ov.ctypes.data + 2, 3, 5, 0, 0, 0.0), b"aligned")]
    refusals += [((1, ov.ctypes.data) + rule, word) for rule, word in OVERLAY_RULES]
    for args, word in refusals:
        _arm(lib)
        assert lib.stm_set_overlay(*args) == -1, args
        err = lib.stm_last_error()
        assert b"set_overlay:" in err and word in err, (args, err)
        assert _overlay(lib) == (1, 3, 5, -2, 7, -13.75), args  # unchanged
    for args in ((1, ov.ctypes.data, 65535, 65535, 65536, -65536, 4096.0), (1, ov.ctypes.data, 1, 1, 0, 0, -4096.0)):
        assert lib.stm_set_overlay(*args) == 0
        assert _overlay(lib) == (args[0],) + args[2:]
    assert lib.stm_set_overlay(0, None, -5, 99, 1 << 20, 7, NAN) == 0  # mode 0: the other arguments are ignored
    assert _overlay(lib) == (0, 0, 0, 0, 0, 0.0)


# the geometry of a stage call: (num_views, angle, lens_mode, pitch, slope, centre, layout, tiles_x, tiles_y, order, out_rows, out_cols, elem_sz)
GOOD = (8, 18.43, 0, 0.0, 0.0, 0.0, 0, 1, 1, 0, 8, 8, 4)


def _geom(**kw):
    names = ("num_views", "angle", "lens_mode", "pitch", "slope", "centre", "layout", "tiles_x", "tiles_y", "order", "out_rows", "out_cols", "elem_sz")
    g = dict(zip(names, GOOD))
    g.update(kw)
    return tuple(g[n] for n in names)


GEOMETRY_RULES = [(_geom(num_views=1), b"num_views"), (_geom(out_rows=0), b"out_rows"), (_geom(out_cols=0), b"out_cols"), (_geom(elem_sz=2), b"elem_sz"),
                  (_geom(lens_mode=4), b"lens mode"), (_geom(lens_mode=-1), b"lens mode"), (_geom(lens_mode=1, pitch=0.5), b"pitch"),
                  (_geom(lens_mode=2, pitch=NAN), b"pitch"), (_geom(lens_mode=3, pitch=7.37, slope=INF), b"slope"),
                  (_geom(lens_mode=3, pitch=7.37, slope=0.86, centre=NAN), b"centre"), (_geom(layout=2), b"layout"),
                  (_geom(layout=1, tiles_x=0, tiles_y=2), b"tiles_x"), (_geom(layout=1, tiles_x=4, tiles_y=0), b"tiles_y"),
                  (_geom(layout=1, tiles_x=4, tiles_y=2, order=4), b"order"), (_geom(layout=1, tiles_x=4, tiles_y=3), b"num_views"),
                  (_geom(layout=1, tiles_x=8, tiles_y=1, out_cols=7), b"out_cols"), (_geom(layout=1, tiles_x=1, tiles_y=8, out_rows=7), b"out_rows"),
                  (_geom(layout=1, tiles_x=4, tiles_y=2, lens_mode=1, pitch=8.0, slope=1.0), b"lens"),
                  (_geom(layout=1, tiles_x=65535, tiles_y=2, num_views=131070, out_rows=2, out_cols=65535), b"65535"),
                  (_geom(angle=0.0), b"angle"), (_geom(angle=NAN), b"angle"), (_geom(angle=89.999), b"too steep")]


def test_stage_rules_are_reported_and_nothing_is_written(lib):
    """both flavours; the frame keeps its fill.  (The device flavour is given host memory: no call gets past the screen.)"""
    frame = np.full((8, 8, 4), 7, np.uint8)
    ov = np.full((3, 5, 4), 9, np.uint8)
    cases = [((3, 5, 0, 0, 0.0) + g, word) for g, word in GEOMETRY_RULES] + [(rule + GOOD, word) for rule, word in OVERLAY_RULES]
    for fn, name in ((lib.stm_mux_overlay, b"mux_overlay"), (lib.stm_d_mux_overlay, b"d_mux_overlay")):
        dev = name.startswith(b"d_")
        fp, op = (frame.ctypes.data, ov.ctypes.data) if dev else (frame.ctypes.data_as(u8p), ov.ctypes.data_as(u8p))
        for args, word in cases:
            _arm(lib)
            fn(fp, op, *args)
            err = lib.stm_last_error()
            # the angle's message is the interlacer's own, as stm_mux_multiview reports it
            assert word in err and ((b" " + name + b":") in (b" " + err).replace(b"\n", b" ") or b"mux_multiview:" in err), (name, args, err)
        _arm(lib)
        fn(fp, None, 3, 5, 0, 0, 0.0, *GOOD)
        assert b"null" in lib.stm_last_error()
    _arm(lib)
    lib.stm_d_mux_overlay(frame.ctypes.data, ov.ctypes.data + 2, 3, 5, 0, 0, 0.0, *GOOD)  # the device flavour reads whole words
    assert b"aligned" in lib.stm_last_error()
    assert (frame == 7).all() and (ov == 9).all()
    assert _overlay(lib) == (0, 0, 0, 0, 0, 0.0)  # the stage does not touch the thread's setting


def test_stage_lens_mode_3_passes_the_screen(lib):
    """mode 3 needs no views: the stage takes it (stm_mux_multiview_lens does not).  An overlay wholly outside the frame has an empty
    bounding box, so the device flavour launches nothing and the call is legal without a GPU."""
    frame = np.full((8, 8, 4), 7, np.uint8)
    ov = np.full((3, 5, 4), 9, np.uint8)
    for geom in (_geom(lens_mode=3, pitch=7.37, slope=0.86, centre=0.3), GOOD, _geom(layout=1, tiles_x=4, tiles_y=2, order=3)):
        for x0, y0 in ((0, 8), (0, -3), (4000, 0), (-4000, 0)):
            _arm(lib)
            lib.stm_d_mux_overlay(frame.ctypes.data, ov.ctypes.data, 3, 5, x0, y0, 2.5, *geom)
            assert b"d_filter_median" in lib.stm_last_error(), (geom, x0, y0)
    assert (frame == 7).all()


def _frame_call(lib, name, stages=3, rows_out=8, cols_out=12, views=8):
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
        if name.endswith("2nv12"):
            lib.stm_d_adcensus_stm_2nv12(None, wsbs, None, wsbs, 0, None, None, None, *reduced, stages, None, None, None, None, 0.5, 24, 1.5, None, None)
        elif name.endswith("2t"):
            lib.stm_d_adcensus_stm_2t(None, None, None, None, *reduced, stages, None, None, None, 0.5, 24, 1.5)
        else:
            getattr(lib, name)(None, None, None, None, *(reduced + ((stages,) if name.endswith("2s") else ())))


FRAME_CALLS = ("stm_d_adcensus_stm", "stm_d_adcensus_stm_t", "stm_d_adcensus_stm_nv12", "stm_adcensus_stm", "stm_adcensus_stm_2",
               "stm_d_adcensus_stm_2", "stm_adcensus_stm_2s", "stm_d_adcensus_stm_2s", "stm_d_adcensus_stm_2t", "stm_d_adcensus_stm_2nv12")


@pytest.mark.parametrize("overlay_first", [True, False], ids=["overlay_then_nv12", "nv12_then_overlay"])
def test_every_frame_call_refuses_nv12_output_with_an_overlay(lib, overlay_first):
    """null pointers throughout: a call that got past the screen would dereference them.  Neither setter refuses the other (each is
    legal on its own); the frame call does, in whichever order the two were set, and leaves both settings as they were."""
    ov = np.zeros((2, 2, 4), np.uint8)
    assert lib.stm_set_layout(1, 4, 2, 0, 1) == 0
    steps = [lambda: lib.stm_set_overlay(1, ov.ctypes.data, 2, 2, 1, 1, 3.0), lambda: lib.stm_set_output(1, 0, 0, 0)]
    for step in (steps if overlay_first else steps[::-1]):
        assert step() == 0
    for name in FRAME_CALLS:
        _arm(lib)
        _frame_call(lib, name)
        err = lib.stm_last_error()
        assert name[4:].encode() + b":" in err and b"overlay" in err and b"NV12" in err, (name, err)
    assert _overlay(lib) == (1, 2, 2, 1, 1, 3.0)
    out = (ctypes.c_int * 4)()
    lib.stm_get_output(out)
    assert tuple(out) == (1, 0, 0, 0)
