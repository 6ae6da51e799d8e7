"""CPU checks of the C boundary of the rectification (include/stm_rectify.h): declared in a header of its own and prototyped in a
table of its own, _lib.PROTOS_RECTIFY -- include/stm_hip.h, _lib.PROTOS and _lib.PROTOS_DEPTH are held to what they were by existing
tests and take no further name --, exported, with the right kinds of argument, usable from plain C and C++, the header stating the
definition, the stream entry outside the setters' recorded table, no thread-level setter exported, and the kernel file a source of the
library.  A frame stream cannot be created without a device, so the entries' refusals are in tests/test_gpu_rectify.py."""
import ctypes
import inspect
import os
import re
import subprocess

from conftest import ROOT

INC = os.path.join(ROOT, "include")
SIGS = {
    "stm_rectify": ("pppiiii", None),
    "stm_d_rectify": ("pppiiii", None),
    "stm_rectify_coords": ("ppii", None),
    "stm_stream_rectify": ("pipi", ctypes.c_int),
    "stm_stream_get_rectify": ("pppp", ctypes.c_int),
}


def _header(name="stm_rectify.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, name)).read(), flags=re.S)


def _declared(name="stm_rectify.h"):
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
    assert sorted(_lib.PROTOS_RECTIFY) == _declared() == sorted(SIGS)
    for name, (sig, res) in SIGS.items():
        args, r = _lib.PROTOS_RECTIFY[name]
        assert "".join(_kind(t) for t in args) == sig and r is res, name
        m = re.search(r"\b(int|void)\s+%s\s*\(([^)]*)\)" % name, _header())
        assert m, name
        kinds = ["p" if "*" in a else "f" if a.split()[0] == "float" else "i" for a in (a.strip() for a in m.group(2).split(","))]
        assert "".join(kinds) == sig and (m.group(1) == "int") == (res is ctypes.c_int), name
    assert '#include "stm_hip.h"' in _header()


def test_the_table_is_disjoint_from_the_other_tables_which_are_as_they_were():
    from stm_amd import _lib
    assert not set(_lib.PROTOS_RECTIFY) & (set(_lib.PROTOS) | set(_lib.PROTOS_DEPTH))
    assert sorted(_lib.PROTOS) == _declared("stm_hip.h") and sorted(_lib.PROTOS_DEPTH) == _declared("stm_depth_input.h")
    assert not [n for n in _declared("stm_hip.h") + _declared("stm_depth_input.h") if "rectif" in n]
    assert "stm_rectify.h" in open(os.path.join(INC, "stm_hip.h")).read()  # the pointing comment


def test_the_library_exports_them_and_no_thread_level_setter(stm):
    out = subprocess.check_output(["nm", "-D", "--defined-only", stm.LIB_PATH]).decode()
    exported = set(re.findall(r"\bT (stm_[a-z0-9_]+)\b", out))
    assert set(SIGS) <= exported
    assert sorted(n for n in exported if "rectif" in n) == sorted(SIGS)  # no stm_set_rectify, no frame entry
    assert "launch_rectify" not in out and "rectify_frame_input" not in out  # internal functions of the library
    lib = stm.lib()  # (loading needs no device)
    for name, (sig, res) in SIGS.items():
        fn = getattr(lib, name)
        assert "".join(_kind(t) for t in fn.argtypes) == sig and fn.restype is res, name


def test_the_stream_entries_are_outside_the_setters_table():
    for name in SIGS:
        assert not name.startswith("stm_stream_set_"), name
    assert sum(name.startswith("stm_stream_") for name in SIGS) == 2


def test_the_header_states_the_definition():
    txt = open(os.path.join(INC, "stm_rectify.h")).read()
    at = txt.index("rectification: an addition")
    body = txt[at:txt.index("void  stm_rectify(", at)]
    for step in ("A. the ray", "B. the distortion", "C. the source position", "D. the taps", "E. the blend"):
        assert step in body, step
    for line in ("X = m00*xf;  t = m01*yf;  X = X + t;  X = X + m02", "xn = X / Wd;  yn = Y / Wd",
                 "rad = k3*r2;  rad = rad + k2;  rad = rad*r2;  rad = rad + k1;  rad = rad*r2;  rad = rad + 1",
                 "mu = u*32;  mu = mu + 0.5;  mu = floorf(mu)", "ok = mu >= -1048576 && mu <= 1048576 && mv >= -1048576 && mv <= 1048576",
                 "out = ((32-fv)*top + fv*bot + 512) >> 10", "m00 m01 m02 m10 m11 m12 m20 m21 m22", "k1 k2 p1 p2 k3"):
        assert line in body, line
    assert "DESIGN.md section 32" in body


def test_the_calls_compile_from_plain_c_and_cxx(tmp_path):
    body = ('#include "stm_rectify.h"\n'
            'int use(void *s, unsigned char *o, const unsigned char *i, int *quv) {\n'
            '    float rec[36] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1};\n'
            '    int mode, border;\n'
            '    stm_rectify(o, i, rec, 4, 6, 3, 0);\n'
            '    stm_d_rectify(o, i, rec, 4, 6, 4, 1);\n'
            '    stm_rectify_coords(quv, rec, 4, 6);\n'
            '    if (stm_stream_rectify(s, 1, rec, 1) != 0) return -1;\n'
            '    stm_stream_destroy(s);  /* the header brings stm_hip.h with it */\n'
            '    return stm_stream_get_rectify(s, &mode, rec, &border);\n'
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


def test_the_kernel_file_is_a_source_of_the_library():
    mk = open(os.path.join(ROOT, "stereo-to-multiview-cuda_amd", "csrc", "Makefile")).read()
    assert "stm_kernels_rectify.hip" in re.search(r"^SRCS\s*:=(.*?)\n(?!\s)", mk, flags=re.S | re.M).group(1)
    assert "-ffp-contract=off" in mk  # the chain's roundings
    assert "stm_rectify.h" in re.search(r"^HDRS\s*:=(.*)$", mk, flags=re.M).group(1)


def test_the_python_surface():
    from stm_amd import device_api, host_api, rectify, video
    assert "rectify" in inspect.signature(video.FrameStream.__init__).parameters
    assert "rectify" in inspect.signature(video.process_sequence).parameters
    for mod, names in ((rectify, ("record", "identity", "inner_rect")), (host_api, ("rectify", "rectify_coords")), (device_api, ("d_rectify",)),
                       (video.FrameStream, ("set_rectify", "get_rectify")), (video, ("take_rectify_option",))):
        for name in names:
            assert callable(getattr(mod, name)), name
