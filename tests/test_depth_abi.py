"""CPU checks of the depth budget's C boundary (stm_set_depth, stm_set_depth_auto, stm_depth_fit / stm_d_depth_fit and the three
frame-stream calls): declared, exported, prototyped, usable from plain C and C++ (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

INC = os.path.join(ROOT, "include")
DEPTH_SYMBOLS = ["stm_set_depth", "stm_set_depth_auto", "stm_depth_fit", "stm_d_depth_fit", "stm_stream_set_depth",
                 "stm_stream_set_depth_auto", "stm_stream_depth"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "stm_hip.h")).read(), flags=re.S)


def test_depth_symbols_are_declared_exported_and_prototyped(stm):
    from stm_amd import _lib
    declared = set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header()))
    lib = ctypes.CDLL(stm.LIB_PATH)
    for name in DEPTH_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOS, name


def test_prototypes_match_the_declarations():
    """argument count and the int / float / pointer kind of every argument, read off the header"""
    from stm_amd import _lib
    txt = _header()
    for name in DEPTH_SYMBOLS:
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


def test_depth_calls_compile_from_plain_c_and_cxx(tmp_path):
    body = ('#include "stm_hip.h"\n'
            'int use(void *s, float *l, float *r, float *st) {\n'
            '    float out[2];\n'
            '    if (stm_set_depth_auto(-4.0f, 4.0f, 1.0f, 20, 1.0f, st) != 0) return -1;\n'
            '    if (stm_set_depth(2, 0.0f, 0.0f) != 0) return -1;\n'
            '    stm_depth_fit(l, r, 1, 1, -4.0f, 4.0f, 1.0f, 20, 1.0f, st);\n'
            '    stm_d_depth_fit(l, r, 1, 1, -4.0f, 4.0f, 1.0f, 20, 1.0f, st);\n'
            '    if (stm_stream_set_depth_auto(s, -4.0f, 4.0f, 1.0f, 20, 0.25f) != 0) return -1;\n'
            '    if (stm_stream_set_depth(s, 2, 0.0f, 0.0f) != 0) return -1;\n'
            '    return stm_stream_depth(s, out);\n'
            '}\n')
    c = tmp_path / "t.c"
    c.write_text(body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-c", str(c), "-o", str(tmp_path / "t.o")])
    cpp = tmp_path / "t.cpp"
    cpp.write_text(body)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", INC, "-c", str(cpp), "-o", str(tmp_path / "u.o")])
    und = subprocess.check_output(["nm", "-u", str(tmp_path / "u.o")]).decode()
    for name in DEPTH_SYMBOLS:
        assert re.search(r"\b%s\b" % name, und), name  # C linkage from C++ too
