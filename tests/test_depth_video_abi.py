"""CPU checks of the C boundary of a frame stream's packed 2D-plus-depth video input (stm_stream_input_packed_depth): declared in a
header of its own, include/stm_depth_video.h, and prototyped in a table of its own, _lib.PROTOS_DEPTH_VIDEO -- include/stm_hip.h,
include/stm_depth_input.h, _lib.PROTOS and _lib.PROTOS_DEPTH are held to what they were by existing tests and take no further name --,
exported, with the right kinds of argument, usable from plain C and C++, a stream entry outside the setters' recorded table and the
only new symbol, the header stating steps 0 and A' to A''', and the Python surface as far as it goes without a GPU.  A frame stream
cannot be created without a device, so the entry's refusals are in tests/test_gpu_depth_video.py."""
import ctypes
import inspect
import os
import re
import subprocess

from conftest import ROOT

INC = os.path.join(ROOT, "include")
NAME, SIG = "stm_stream_input_packed_depth", "piiiiiiiiiffif"


def _header(name="stm_depth_video.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, name)).read(), flags=re.S)


def _declared(name="stm_depth_video.h"):
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
    assert sorted(_lib.PROTOS_DEPTH_VIDEO) == _declared() == [NAME]
    args, res = _lib.PROTOS_DEPTH_VIDEO[NAME]
    assert "".join(_kind(t) for t in args) == SIG and res is ctypes.c_int
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, _header())
    assert m
    kinds = ["p" if "*" in a else "f" if a.split()[0] == "float" else "i" for a in (a.strip() for a in m.group(1).split(","))]
    assert "".join(kinds) == SIG
    names = [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["stream", "format", "matrix", "packing", "swap", "filter", "gap", "range", "dfilter", "dgate", "lo", "hi", "fill", "gate"]
    assert '#include "stm_hip.h"' in _header()


def test_the_other_tables_and_headers_are_as_they_were():
    from stm_amd import _lib
    others = set(_lib.PROTOS) | set(_lib.PROTOS_DEPTH) | set(_lib.PROTOS_RECTIFY) | set(_lib.PROTOS_HSLO)
    assert not set(_lib.PROTOS_DEPTH_VIDEO) & others
    assert sorted(_lib.PROTOS) == _declared("stm_hip.h") and sorted(_lib.PROTOS_DEPTH) == _declared("stm_depth_input.h") == ["stm_stream_input_depth"]
    assert not [n for n in _declared("stm_hip.h") + _declared("stm_depth_input.h") if "packed_depth" in n or "depth_video" in n]
    for other in ("stm_hip.h", "stm_depth_input.h"):  # the pointing comments
        assert "stm_depth_video.h" in open(os.path.join(INC, other)).read(), other


def test_the_library_exports_it_and_nothing_else_of_the_feature(stm):
    out = subprocess.check_output(["nm", "-D", "--defined-only", stm.LIB_PATH]).decode()
    exported = set(re.findall(r"\bT (stm_[a-z0-9_]+)\b", out))
    assert NAME in exported
    assert sorted(n for n in exported if "packed_depth" in n or "depth_video" in n or "eye" in n) == [NAME]  # no stage call, no frame entry
    assert "depth_video_frame_device" not in out and "launch_depth_eye_video" not in out  # internal functions of the library
    fn = getattr(stm.lib(), NAME)  # (loading needs no device)
    assert "".join(_kind(t) for t in fn.argtypes) == SIG and fn.restype is ctypes.c_int


def test_it_is_a_stream_entry_outside_the_setters_table():
    assert NAME.startswith("stm_stream_") and not NAME.startswith("stm_stream_set_")


def test_the_header_states_the_definition():
    txt = open(os.path.join(INC, "stm_depth_video.h")).read()
    at = txt.index("packed 2D-plus-depth input: the stream's frames")
    body = txt[at:txt.index("stm_stream_input_packed_depth(void", at)]
    for step in ("0.    the image", "A'.   the depth sample", "A''.  expansion", "A'''. decode", "B to F."):
        assert step in body, step
    for line in ("c = min(max(sample, 16), 235) - 16;    M = 219", "c = sample;                            M = 255",
                 "k = a >> 1;  s = +1 if a is odd else -1;  n = clamp(k + s, 0, last)", "c0 = c(P[k]);  c1 = c(P[n])",
                 "dfilter 0:  v = 4 c0", "dfilter 1:  v = |c0 - c1| <= dgate ? 3 c0 + c1 : 4 c0",
                 "q4 = (float)(((double)hi - (double)lo) / (4.0 * M))", "t = (float)v * q4", "d = lo + t",
                 "sample = the Y byte at (row, col)", "sample = byte 1 (G) of the pixel at (row, col)"):
        assert line in body, line
    assert "DESIGN.md section 34" in body and "stream_input_packed_depth" in body


def test_the_call_compiles_from_plain_c_and_cxx(tmp_path):
    body = ('#include "stm_depth_video.h"\n'
            'int use(void *s) {\n'
            '    if (stm_stream_input_packed_depth(s, 1, 1, 1, 0, 1, 0, 1, 1, 4, 12.0f, -12.0f, 1, 0.5f) != 0) return -1;\n'
            '    stm_stream_destroy(s);  /* the header brings stm_hip.h with it */\n'
            '    return stm_stream_input_packed_depth(0, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0.0f, 0.0f, 0, 0.0f);\n'
            '}\n')
    c = tmp_path / "t.c"
    c.write_text(body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-c", str(c), "-o", str(tmp_path / "t.o")])
    cpp = tmp_path / "t.cpp"
    cpp.write_text(body)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", INC, "-c", str(cpp), "-o", str(tmp_path / "u.o")])
    assert re.search(r"\b%s\b" % NAME, subprocess.check_output(["nm", "-u", str(tmp_path / "u.o")]).decode())  # C linkage from C++ too


def test_the_kernel_is_in_the_eye_file_and_the_header_a_dependency():
    csrc = os.path.join(ROOT, "stereo-to-multiview-cuda_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "stm_depth_video.h" in re.search(r"^HDRS\s*:=(.*)$", mk, flags=re.M).group(1) and "-ffp-contract=off" in mk
    eye = open(os.path.join(csrc, "stm_kernels_eye.hip")).read()
    assert "void stm_k_eye_video(" in eye and "void stm_k_eye(EyeArgs a)" in eye


def test_the_python_surface():
    from stm_amd import video
    assert "depth_video" in inspect.signature(video.FrameStream.__init__).parameters
    assert "depth_video" in inspect.signature(video.process_sequence).parameters
    assert callable(video.FrameStream.set_depth_video) and callable(video.take_depth_video_option)
    want = ["self", "format", "matrix", "packing", "swap", "filter", "gap", "range", "dfilter", "dgate", "lo", "hi", "fill", "gate"]
    assert list(inspect.signature(video.FrameStream.set_depth_video).parameters) == want
