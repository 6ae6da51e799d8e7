"""CPU checks of the C boundary of include/stm_hslo_tap.h -- the test tap on the scanline passes' path-cost sums (stm_set_hslo_tap) and
scanline optimisation of either view as a stage (stm_d_dc_hslo_view): declared in a header of its own and prototyped in a table of
its own, _lib.PROTOS_HSLO -- include/stm_hip.h, _lib.PROTOS, PROTOS_DEPTH and PROTOS_RECTIFY are held to what they were by existing
tests and take no further name --, exported, with the right kinds of argument, usable from plain C and C++, and what the two calls
refuse before they touch the device, text for text.  What the calls compute is in tests/test_gpu_hslo_sums.py."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "include")
SIGS = {
    "stm_set_hslo_tap": ("ppp", ctypes.c_int),
    "stm_d_dc_hslo_view": ("ppppfffiiiiii", None),
}


def _header(name="stm_hslo_tap.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, name)).read(), flags=re.S)


def _declared(name="stm_hslo_tap.h"):
    return sorted(set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header(name))))


def _kind(t):
    if t is ctypes.c_int:
        return "i"
    if t is ctypes.c_float:
        return "f"
    assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), t
    return "p"


def test_the_table_and_the_header_are_held_to_each_other():
    from stm_amd import _lib
    assert sorted(_lib.PROTOS_HSLO) == _declared() == sorted(SIGS)
    for name, (sig, res) in SIGS.items():
        args, r = _lib.PROTOS_HSLO[name]
        assert "".join(_kind(t) for t in args) == sig and r is res, name
        m = re.search(r"\b(int|void)\s+%s\s*\(([^)]*)\)" % name, _header())
        assert m, name
        kinds = ["p" if "*" in a else "f" if a.split()[0] == "float" else "i" for a in (a.strip() for a in m.group(2).split(","))]
        assert "".join(kinds) == sig and (m.group(1) == "int") == (res is ctypes.c_int), name
    assert '#include "stm_hip.h"' in _header()


def test_the_view_entry_takes_d_dc_hslos_arguments_and_a_view():
    from stm_amd import _lib
    args, res = _lib.PROTOS["stm_d_dc_hslo"]
    vargs, vres = _lib.PROTOS_HSLO["stm_d_dc_hslo_view"]
    assert [_kind(t) for t in vargs] == [_kind(t) for t in args] + ["i"] and vres is res
    m = re.search(r"\bstm_d_dc_hslo_view\s*\(([^)]*)\)", _header())
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")][-6:] == ["num_disp", "zero_disp", "num_rows", "num_cols", "elem_sz", "view"]


def test_the_table_is_disjoint_from_the_other_tables_which_are_as_they_were():
    from stm_amd import _lib
    others = set(_lib.PROTOS) | set(_lib.PROTOS_DEPTH) | set(_lib.PROTOS_RECTIFY)
    assert not set(_lib.PROTOS_HSLO) & others
    assert sorted(_lib.PROTOS) == _declared("stm_hip.h") and sorted(_lib.PROTOS_DEPTH) == _declared("stm_depth_input.h")
    assert sorted(_lib.PROTOS_RECTIFY) == _declared("stm_rectify.h")
    assert not [n for n in others if "hslo_tap" in n or "hslo_view" in n]
    assert "stm_hslo_tap.h" in open(os.path.join(INC, "stm_hip.h")).read()  # the pointing comment


def test_the_library_exports_them(stm):
    out = subprocess.check_output(["nm", "-D", "--defined-only", stm.LIB_PATH]).decode()
    exported = set(re.findall(r"\bT (stm_[a-z0-9_]+)\b", out))
    assert set(SIGS) <= exported
    assert sorted(n for n in exported if "hslo" in n) == sorted(list(SIGS) + ["stm_dc_hslo", "stm_d_dc_hslo"])
    assert "launch_hslo" not in out  # internal functions of the library
    lib = stm.lib()  # (loading needs no device)
    for name, (sig, res) in SIGS.items():
        fn = getattr(lib, name)
        assert "".join(_kind(t) for t in fn.argtypes) == sig and fn.restype is res, name


def test_the_header_says_what_the_tap_holds_and_that_a_stream_never_runs_it():
    txt = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(INC, "stm_hslo_tap.h")).read())  # comment lines joined
    for line in ("[views][D][H][W] float32", "C_lr + C_rl", "(C_lr + C_rl) + C_tb", "(((C_lr + C_rl) + C_tb) + C_bt) * 0.25f",
                 "image columns only", "the same kernel that runs with the tap clear", "no launch is added",
                 "A frame stream refuses stages bit 0x100, so a stream never runs the tap", "x - (d - zero_disp)"):
        assert line in txt, line


def test_the_calls_compile_from_plain_c_and_cxx(tmp_path):
    body = ('#include "stm_hslo_tap.h"\n'
            'int use(float **tab, float *vol, float *disp, unsigned char *own, unsigned char *other) {\n'
            '    if (stm_set_hslo_tap(vol, 0, vol) != 0) return -1;\n'
            '    stm_d_dc_hslo_view(tab, disp, own, other, 15.0f, 1.0f, 3.0f, 20, 7, 4, 6, 3, 1);\n'
            '    stm_d_dc_hslo(tab, disp, own, other, 15.0f, 1.0f, 3.0f, 20, 7, 4, 6, 3);  /* the header brings stm_hip.h with it */\n'
            '    return stm_set_hslo_tap(0, 0, 0);\n'
            '}\n')
    c = tmp_path / "t.c"
    c.write_text(body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-c", str(c), "-o", str(tmp_path / "t.o")])
    cpp = tmp_path / "t.cpp"
    cpp.write_text(body)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", INC, "-c", str(cpp), "-o", str(tmp_path / "u.o")])
    undefined = subprocess.check_output(["nm", "-u", str(tmp_path / "u.o")]).decode()
    for name in SIGS:
        assert re.search(r"\b%s\b" % name, undefined), name  # C linkage from C++ too


def test_the_header_is_a_dependency_of_the_library():
    mk = open(os.path.join(ROOT, "stereo-to-multiview-cuda_amd", "csrc", "Makefile")).read()
    assert "stm_hslo_tap.h" in re.search(r"^HDRS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert "-ffp-contract=off" in mk  # the sums' roundings


@pytest.fixture
def lib(stm):
    lib = stm.lib()
    lib.stm_set_error_mode(1)
    try:
        yield lib
    finally:
        lib.stm_set_error_mode(0)


def _said(lib):
    return lib.stm_last_error().decode().split("\n", 1)[1]  # (the first line is the refusing rule's file:line; the argument's name ends the text)


P = 0x10000  # a dummy address: every call below is refused before anything looks behind a pointer


def test_the_taps_refusals(lib):
    for k, name in enumerate(("d_s2", "d_s3", "d_fin")):
        for off in (1, 2, 3):
            a = [P, P, P]
            a[k] = P + off
            assert lib.stm_set_hslo_tap(*a) == -1
            assert _said(lib) == "set_hslo_tap: %s must be 4-byte aligned (a volume of floats) %s" % (name, name)
    assert lib.stm_set_hslo_tap(P + 1, P + 2, P) == -1 and _said(lib).startswith("set_hslo_tap: d_s2 ")  # the first broken one is named
    assert lib.stm_set_hslo_tap(None, None, None) == 0  # nothing was set on the way, and clearing is never refused


def test_the_view_entrys_refusals(lib):
    good = dict(num_disp=20, zero_disp=7, num_rows=4, num_cols=6, elem_sz=3, view=1)

    def call(**over):
        a = dict(good, **over)
        lib.stm_d_filter_median(None, 0, 0)  # plant a known message: a call that records nothing shows this one
        lib.stm_d_dc_hslo_view(P, P, P, P, 15.0, 1.0, 3.0, a["num_disp"], a["zero_disp"], a["num_rows"], a["num_cols"], a["elem_sz"], a["view"])
        return _said(lib)

    # the dimension screen is stm_d_dc_hslo's, under the entry's own name
    assert call(num_disp=0) == "d_dc_hslo_view: num_disp = 0, must be >= 1 num_disp"
    assert call(num_rows=0) == "d_dc_hslo_view: num_rows = 0, must be >= 1 num_rows"
    assert call(num_cols=-5) == "d_dc_hslo_view: num_cols = -5, must be >= 1 num_cols"
    assert call(elem_sz=2) == "d_dc_hslo_view: elem_sz = 2, must be >= 3 elem_sz"
    lib.stm_d_filter_median(None, 0, 0)
    lib.stm_d_dc_hslo(P, P, P, P, 15.0, 1.0, 3.0, 20, 7, 4, 6, 2)
    assert _said(lib) == "d_dc_hslo: elem_sz = 2, must be >= 3 elem_sz"
    # then the view
    assert call(view=2) == "d_dc_hslo_view: view = 2, must be 0 (the left view) or 1 (the right view) view"
    assert call(view=-1) == "d_dc_hslo_view: view = -1, must be 0 (the left view) or 1 (the right view) view"
    assert call(view=2, num_rows=0) == "d_dc_hslo_view: num_rows = 0, must be >= 1 num_rows"  # the dimensions win


def test_the_python_surface():
    from stm_amd import device_api
    for name in ("set_hslo_tap", "hslo_tap", "d_dc_hslo_view"):
        assert callable(getattr(device_api, name)), name
    from oracle import pyoracle
    assert callable(pyoracle.dc_hslo_sums)
