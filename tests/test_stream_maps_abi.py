"""CPU checks of the C boundary of a frame stream's map formats (stm_stream_maps, stm_stream_collect_maps,
stm_stream_collect_maps_view): declared, exported, prototyped with the right kinds of argument, usable from plain C and C++ -- and
nothing else new in the header: the quantiser has no per-stage call.  A frame stream cannot be created
without a device: the calls' rules are in tests/test_gpu_stream_maps.py.  Also the Python surface and the driver's option, as far as
they go without a GPU."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

INC = os.path.join(ROOT, "include")
SIGNATURES = {"stm_stream_maps": "piiff", "stm_stream_collect_maps": "pppp", "stm_stream_collect_maps_view": "pppp"}
RESULTS = {"stm_stream_maps": ctypes.c_int, "stm_stream_collect_maps": ctypes.c_long, "stm_stream_collect_maps_view": ctypes.c_long}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "stm_hip.h")).read(), flags=re.S)


def _kind(t):
    if t is ctypes.c_int:
        return "i"
    if t is ctypes.c_float:
        return "f"
    assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), t
    return "p"


def test_the_three_entries_are_prototyped():
    from stm_amd import _lib
    for name, sig in SIGNATURES.items():
        assert name in _lib.PROTOS, name
        args, res = _lib.PROTOS[name]
        assert "".join(_kind(t) for t in args) == sig, name
        assert res is RESULTS[name], name


def test_the_library_exports_them(stm):
    out = subprocess.check_output(["nm", "-D", "--defined-only", stm.LIB_PATH]).decode()
    exported = set(re.findall(r"\bT (stm_[a-z0-9_]+)\b", out))
    assert set(SIGNATURES) <= exported


def test_the_declarations_are_as_prototyped():
    """argument count and the int / float / pointer kind of every argument, read off the header"""
    txt = _header()
    for name, sig in SIGNATURES.items():
        m = re.search(r"\b(int|long)\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        kinds = ["p" if "*" in a else "f" if a.split()[0] == "float" else "i" for a in (a.strip() for a in m.group(2).split(","))]
        assert "".join(kinds) == sig, name
        assert m.group(1) == ("int" if RESULTS[name] is ctypes.c_int else "long"), name


def test_the_header_declares_nothing_else_new():
    """every symbol of the header is one the screening tables knew before this feature, or one of the three: the generator of
    tests/golden/entry_screening.json names every earlier entry in one of its groups"""
    spec = importlib.util.spec_from_file_location("make_entry_screening", os.path.join(GOLDEN, "make_entry_screening.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    declared = set(re.findall(r"\b(stm_[a-z0-9_]+)\s*\(", _header()))
    # the stream entries that refuse no setting (create, submit, collect, the readers ...) are in no table: the header had these
    before = {"stm_stream_create", "stm_stream_submit", "stm_stream_collect", "stm_stream_collect_view", "stm_stream_input_buffer",
              "stm_stream_destroy", "stm_stream_depth", "stm_stream_align", "stm_stream_balance", "stm_stream_cut", "stm_stream_active",
              "stm_stream_overlay_depth"}
    known = set(gen.ENTRIES) | set(gen.FRAME_ENTRIES) | set(gen.NO_SCREEN) | set(gen.STREAM_SETTERS) | before
    assert declared - known == set(SIGNATURES), sorted(declared - known)
    assert not [n for n in SIGNATURES if n.startswith("stm_stream_set_")]  # a stream setting, but no member of the setters' table


def test_calls_compile_from_plain_c_and_cxx(tmp_path):
    body = ('#include "stm_hip.h"\n'
            'long use(void *s, unsigned short *l, unsigned char *frame) {\n'
            '    const void *vl, *vr;\n'
            '    const unsigned char *vf;\n'
            '    if (stm_stream_maps(s, 3, 0, 64.0f, 0.0f) != 0) return -1;\n'
            '    if (stm_stream_collect_maps(s, l, 0, frame) < 0) return -1;\n'
            '    return stm_stream_collect_maps_view(s, &vl, &vr, &vf);\n'
            '}\n')
    c = tmp_path / "t.c"
    c.write_text(body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-c", str(c), "-o", str(tmp_path / "t.o")])
    cpp = tmp_path / "t.cpp"
    cpp.write_text(body)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", INC, "-c", str(cpp), "-o", str(tmp_path / "u.o")])
    und = subprocess.check_output(["nm", "-u", str(tmp_path / "u.o")]).decode()
    for name in SIGNATURES:
        assert re.search(r"\b%s\b" % name, und), name  # C linkage from C++ too


def test_the_kernel_file_is_a_source_of_the_library():
    mk = open(os.path.join(ROOT, "stereo-to-multiview-cuda_amd", "csrc", "Makefile")).read()
    assert "stm_kernels_dplane.hip" in re.search(r"^SRCS\s*:=(.*?)\n(?!\s)", mk, flags=re.S | re.M).group(1)
    assert "-ffp-contract=off" in mk  # the definition's two roundings


# ----------------------------------------------------------------------------- Python and the driver
def test_framestream_takes_maps():
    from stm_amd import video
    assert "maps" in inspect.signature(video.FrameStream.__init__).parameters
    assert "maps" in inspect.signature(video.process_sequence).parameters
    assert callable(video.FrameStream.set_maps)


def test_take_maps_option():
    from stm_amd import video
    argv = ["x", "--maps", "u16", "left", "12.5", "-3", "planes.raw", "--cut"]
    assert video.take_maps_option(argv) == ("u16", "left", 12.5, -3.0, "planes.raw") and argv == ["x", "--cut"]
    argv = ["x", "--maps", "u8", "both", "0", "16", "--cut"]
    assert video.take_maps_option(argv) == ("u8", "both", 0.0, 16.0, None) and argv == ["x", "--cut"]
    argv = ["--maps", "none", "y"]
    assert video.take_maps_option(argv) == ("none", "both", 0.0, 0.0, None) and argv == ["y"]
    assert video.take_maps_option(["x"]) is None
    for bad in (["--maps"], ["--maps", "u4", "both", "0", "1"], ["--maps", "u8", "both", "0"], ["--maps", "u8", "all", "0", "1"],
                ["--maps", "u8", "both", "1", "1"], ["--maps", "u8", "both", "nan", "1"], ["--maps", "u16", "both", "0", "5000"],
                ["--maps", "u8", "both", "x", "1"]):
        with pytest.raises((ValueError, IndexError)):
            video.take_maps_option(list(bad))


def test_stm_video_refuses_a_malformed_maps_option(capsys):
    spec = importlib.util.spec_from_file_location("stm_video", os.path.join(ROOT, "tools", "stm_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for tail in (["--maps"], ["--maps", "u12", "both", "0", "16"], ["--maps", "u8", "both", "3", "3"], ["--maps", "u8", "up", "0", "16"]):
        assert mod.main(["stm_video"] + ["x"] * 16 + tail) == -1, tail
        assert "--maps FORMAT" in capsys.readouterr().out
