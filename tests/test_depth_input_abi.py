"""CPU checks of the C boundary of a frame stream's image-plus-depth input (stm_stream_input_depth): declared in a header of its
own, include/stm_depth_input.h, and prototyped in a table of its own, _lib.PROTOS_DEPTH -- include/stm_hip.h and _lib.PROTOS are held
to the recorded screening tables by existing tests and take no further name --, exported, with the right kinds of argument, usable
from plain C and C++, a stream entry that is no member of the setters' recorded table, and the only new symbol: the second eye has no
stage call and no frame entry.  A frame stream cannot be created
without a device, so the entry's refusals are in tests/test_gpu_depth_input.py.  Also the Python surface, as far as it goes without
a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

from conftest import ROOT

INC = os.path.join(ROOT, "include")
NAME, SIG = "stm_stream_input_depth", "piffif"


def _header(name="stm_depth_input.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, name)).read(), flags=re.S)


def _declared(name="stm_depth_input.h"):
    return sorted(set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header(name))))


def _kind(t):
    if t is ctypes.c_int:
        return "i"
    if t is ctypes.c_float:
        return "f"
    assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), t
    return "p"


def test_the_entry_is_prototyped():
    from stm_amd import _lib
    assert NAME in _lib.PROTOS_DEPTH and NAME not in _lib.PROTOS
    args, res = _lib.PROTOS_DEPTH[NAME]
    assert "".join(_kind(t) for t in args) == SIG and res is ctypes.c_int


def test_the_new_table_covers_the_new_header_and_the_old_pair_is_as_it_was():
    """what tests/test_abi.py asks of stm_hip.h and PROTOS, asked of the new header and its table; and the old header names nothing
    of this feature outside its comments"""
    from stm_amd import _lib
    assert sorted(_lib.PROTOS_DEPTH) == _declared() == [NAME]
    assert not set(_lib.PROTOS_DEPTH) & set(_lib.PROTOS)
    assert NAME not in _declared("stm_hip.h") and sorted(_lib.PROTOS) == _declared("stm_hip.h")
    assert '#include "stm_hip.h"' in _header()


def test_the_loaded_library_has_the_prototype(stm):
    fn = stm.lib().stm_stream_input_depth  # (loading needs no device)
    assert "".join(_kind(t) for t in fn.argtypes) == SIG and fn.restype is ctypes.c_int


def test_the_library_exports_it(stm):
    out = subprocess.check_output(["nm", "-D", "--defined-only", stm.LIB_PATH]).decode()
    assert NAME in set(re.findall(r"\bT (stm_[a-z0-9_]+)\b", out))


def test_the_declaration_is_as_prototyped():
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, _header())
    assert m
    kinds = ["p" if "*" in a else "f" if a.split()[0] == "float" else "i" for a in (a.strip() for a in m.group(1).split(","))]
    assert "".join(kinds) == SIG


def test_it_is_a_stream_entry_outside_the_setters_table(stm):
    """the recorded screening tables stay as they are: the name starts with stm_stream_, not with stm_stream_set_, and no stage call
    or stm_d_ frame entry came with it"""
    assert NAME.startswith("stm_stream_") and not NAME.startswith("stm_stream_set_")
    declared = set(_declared()) | set(_declared("stm_hip.h"))
    assert not [n for n in declared if "eye" in n or ("depth_input" in n) or (n != NAME and "input_depth" in n)]
    out = subprocess.check_output(["nm", "-D", "--defined-only", stm.LIB_PATH]).decode()
    assert "depth_frame_device" not in out and "launch_depth_eye" not in out  # internal functions of the library


def test_the_header_states_the_definition():
    txt = open(os.path.join(INC, "stm_depth_input.h")).read()
    at = txt.index("image-plus-depth input: the stream's frames")
    body = txt[at:txt.index("stm_stream_input_depth(void", at)]
    for step in ("A. decode", "B. landing", "C. winner", "D. hit pixels", "E. holes", "F. the frame"):
        assert step in body, step
    assert "DESIGN.md section 31" in body


def test_the_call_compiles_from_plain_c_and_cxx(tmp_path):
    body = ('#include "stm_depth_input.h"\n'
            'int use(void *s) {\n'
            '    if (stm_stream_input_depth(s, 2, 12.0f, -12.0f, 1, 0.5f) != 0) return -1;\n'
            '    stm_stream_destroy(s);  /* the header brings stm_hip.h with it */\n'
            '    return stm_stream_input_depth(0, -1, 0.0f, 0.0f, 0, 0.0f);\n'
            '}\n')
    c = tmp_path / "t.c"
    c.write_text(body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-c", str(c), "-o", str(tmp_path / "t.o")])
    cpp = tmp_path / "t.cpp"
    cpp.write_text(body)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", INC, "-c", str(cpp), "-o", str(tmp_path / "u.o")])
    assert re.search(r"\b%s\b" % NAME, subprocess.check_output(["nm", "-u", str(tmp_path / "u.o")]).decode())  # C linkage from C++ too


def test_the_kernel_file_is_a_source_of_the_library():
    mk = open(os.path.join(ROOT, "stereo-to-multiview-cuda_amd", "csrc", "Makefile")).read()
    assert "stm_kernels_eye.hip" in re.search(r"^SRCS\s*:=(.*?)\n(?!\s)", mk, flags=re.S | re.M).group(1)
    assert "-ffp-contract=off" in mk  # the decode's two roundings


def test_the_python_surface():
    from stm_amd import video
    assert "depth_input" in inspect.signature(video.FrameStream.__init__).parameters
    assert "depth_input" in inspect.signature(video.process_sequence).parameters
    for name in ("set_depth_input", "pack_depth_frame", "submit_depth"):
        assert callable(getattr(video.FrameStream, name)), name
