"""The numpy statement of a frame stream's image-plus-depth input (stm_stream_input_depth; include/stm_depth_input.h states steps A to E line
by line, DESIGN.md section 31 gives the reasons) and its known answers.  No GPU: tests/test_gpu_depth_input.py compares the kernel
with decode_ref and eye_ref bit for bit, and imports the scene from here."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from test_stream_maps_ref import DTYPE, MAXCODE, plane_ref

f32 = np.float32
LIMITS = [(-12.0, 12.0), (12.0, -12.0), (-7.3, 21.9), (0.0, 64.0), (100.1, -3.7), (-4096.0, 4096.0), (0.0, 1.0 / 64.0)]
PLANE_DTYPE = {"f32": np.dtype("<f4"), "u8": DTYPE["u8"], "u16": DTYPE["u16"]}


def decode_ref(plane, fmt, lo, hi):
    """Step A on a whole plane, one float32 operation per line.  Returns the float32 map disp_l."""
    lo, hi = f32(lo), f32(hi)
    if fmt == "f32":
        dmin, dmax = np.fmin(lo, hi), np.fmax(lo, hi)
        t = np.fmin(np.asarray(plane, dtype=f32), dmax)  # fmin returns its other operand for a NaN
        return np.fmax(t, dmin)
    q = f32((float(hi) - float(lo)) / float(MAXCODE[fmt]))
    t = np.asarray(plane).astype(f32) * q
    return (lo + t).astype(f32)


COUNTS = ("collisions", "ties", "two_sided", "one_sided", "background_ties", "mirrors_taken", "mirrors_rejected", "clamped_left", "clamped_right")


def eye_ref(img, disp_l, fill, gate):
    """Steps B to E, serially.  img [H][>= W][>= 3] u8, disp_l [H][W] f32.  Returns (img_r [H][W][3], disp_r, hole mask, counts);
    the two mirror counts are those of fill 1 with this gate, whichever fill is asked for."""
    disp_l = np.asarray(disp_l, dtype=f32)
    H, W = disp_l.shape
    gate = f32(gate)
    img_r = np.zeros((H, W, 3), np.uint8)
    disp_r = np.zeros((H, W), f32)
    holes = np.zeros((H, W), bool)
    n = dict.fromkeys(COUNTS, 0)
    for y in range(H):
        win = [-1] * W
        for x in range(W):
            d = disp_l[y, x]
            c = x + int(d)  # int() truncates as C does
            n["clamped_left"] += c < 0
            n["clamped_right"] += c > W - 1
            c = min(max(c, 0), W - 1)
            if win[c] >= 0:
                n["collisions"] += 1
                n["ties"] += d == disp_l[y, win[c]]
            if win[c] < 0 or d <= disp_l[y, win[c]]:
                win[c] = x
        for c in range(W):
            if win[c] >= 0:
                disp_r[y, c] = disp_l[y, win[c]]
                img_r[y, c] = img[y, win[c], :3]
        k = 0
        while k < W:
            if win[k] >= 0:
                k += 1
                continue
            a = k
            while k < W and win[k] < 0:
                k += 1
            b = k - 1
            L, R = (a - 1 if a > 0 else None), (b + 1 if b < W - 1 else None)
            assert L is not None or R is not None
            if L is not None and R is not None:
                n["two_sided"] += 1
                n["background_ties"] += disp_r[y, L] == disp_r[y, R]
                B = L if disp_r[y, L] > disp_r[y, R] else R
            else:
                n["one_sided"] += 1
                B = L if L is not None else R
            for j in range(a, b + 1):
                holes[y, j] = True
                disp_r[y, j] = disp_r[y, B]
                m = 2 * B - j
                ok = 0 <= m < W and win[m] >= 0 and np.abs(f32(disp_r[y, m] - disp_r[y, B])) <= gate
                n["mirrors_taken" if ok else "mirrors_rejected"] += 1
                img_r[y, j] = img_r[y, m] if fill == 1 and ok else img_r[y, B]
    return img_r, disp_r, holes, n


def scene_disp(H, W, k=0):
    """The test scene's float map, frame k: a far wall 3.25 + 0.03 x on the left half and a flat 3.0 on the right half; a near box at
    -4.5 over columns W/3 .. W/3 + W/4, moved two pixels a frame; a five-column pole at -9.0 on the flat wall (at W = 300 it starts
    at column 254); -6.0 in the first three columns; 7.75 in the last three rows."""
    x = np.arange(W, dtype=f32)
    d = np.where(x < W // 2, f32(3.25) + f32(0.03) * x, f32(3.0)).astype(f32)
    d = np.tile(d, (H, 1))
    x0 = W // 3 + 2 * k
    d[1:H - 1, x0:x0 + W // 4] = -4.5
    p0 = 254 * W // 300
    d[:, p0:p0 + 5] = -9.0
    d[:, :3] = -6.0
    d[H - 3:, :] = 7.75
    return d


def scene_image(H, W, pitch=None, elem_sz=3, seed=5):
    pitch = W if pitch is None else pitch
    return np.random.RandomState(seed * 100003 + H * 1000 + W).randint(0, 256, size=(H, pitch, elem_sz)).astype(np.uint8)


def scene_plane(H, W, fmt, lo, hi, k=0):
    """the scene as a plane of `fmt`: the float map itself (with values beyond both limits and a NaN), or its codes under (lo, hi)"""
    d = scene_disp(H, W, k)
    if fmt == "f32":
        d = d.copy()
        d[0, W // 2] = np.nan
        return d
    return plane_ref(d, fmt, lo, hi)


# ----------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("shift", [4, -3, 0])
def test_a_constant_map_shifts_the_image(shift):
    H, W = 5, 23
    img = scene_image(H, W)
    img_r, disp_r, holes, n = eye_ref(img, np.full((H, W), shift, f32), 0, 0.0)
    assert (disp_r == shift).all()
    lo, hi = max(shift, 0), W + min(shift, 0)
    assert np.array_equal(img_r[:, lo + (shift < 0):hi - (shift > 0)], img[:, lo - shift + (shift < 0):hi - shift - (shift > 0)])
    if shift > 0:  # nothing lands on columns 0 .. shift - 1: one run at the left border, filled from its only neighbour
        assert holes[:, :shift].all() and not holes[:, shift:].any() and n["one_sided"] == H and n["two_sided"] == 0
        assert (img_r[:, :shift] == img_r[:, shift:shift + 1]).all()
    elif shift < 0:  # the clamp at column 0 takes the sources 0 .. -shift: the largest x wins; the run at the right border
        assert holes[:, W + shift:].all() and not holes[:, :W + shift].any() and n["one_sided"] == H
        assert np.array_equal(img_r[:, 0], img[:, -shift]) and (img_r[:, W + shift:] == img_r[:, W + shift - 1:W + shift]).all()
        assert n["ties"] == n["collisions"] == -shift * H
    else:
        assert not holes.any() and np.array_equal(img_r, img)


def test_fill_1_mirrors_a_border_run_about_its_only_neighbour():
    """c(x) = x + 4 never reaches columns 0 .. 3; the clamp at the right border collects the last five sources and the largest x wins"""
    H, W = 3, 16
    img = scene_image(H, W)
    img_r, disp_r, holes, n = eye_ref(img, np.full((H, W), 4, f32), 1, 0.5)
    assert holes[:, :4].all() and holes.sum() == 4 * H and n["one_sided"] == H
    assert np.array_equal(img_r[:, 4:W - 1], img[:, :W - 5]) and np.array_equal(img_r[:, W - 1], img[:, W - 1])
    assert n["clamped_right"] == 4 * H and n["ties"] == 4 * H
    assert np.array_equal(img_r[:, :4], img_r[:, 8:4:-1])  # fill 1 mirrors about B = 4: column k takes column 8 - k


@pytest.mark.parametrize("shape", [(9, 37), (16, 64), (21, 83), (5, 300)])
def test_holes_are_the_renderers_unhit_pixels_and_winners_pass_the_left_check(orc, shape):
    H, W = shape
    d = decode_ref(scene_plane(H, W, "f32", -12.0, 12.0), "f32", -12.0, 12.0)
    img_r, disp_r, holes, n = eye_ref(scene_image(H, W), d, 1, 0.5)
    occl_l, occl_r = orc.dibr_occl(d, disp_r)
    assert np.array_equal(holes, occl_r == 0)
    out_l, _ = orc.dr_dcc(d, disp_r)
    c = np.clip(np.arange(W)[None, :] + d.astype(np.int32), 0, W - 1)
    won = np.take_along_axis(disp_r, c, axis=1) == d  # the pixel's own value stands where it landed
    assert won.any() and not out_l[won].any()


@pytest.mark.parametrize("shape", [(9, 37), (16, 64), (21, 83), (5, 300)])
def test_the_scene_meets_every_case(shape):
    """the conditions tests/test_gpu_depth_input.py relies on: every case of steps B to E occurs, in the float scene and in its codes"""
    H, W = shape
    for fmt, lo, hi in (("f32", -12.0, 12.0), ("u8", 12.0, -12.0), ("u16", -12.0, 12.0)):
        d = decode_ref(scene_plane(H, W, fmt, lo, hi), fmt, lo, hi)
        n = eye_ref(scene_image(H, W), d, 1, 0.5)[3]
        need = [c for c in COUNTS if not (c == "mirrors_rejected" and W > 64)]
        assert all(n[c] > 0 for c in need), (shape, fmt, n)


@pytest.mark.parametrize("fmt", ["u8", "u16"])
@pytest.mark.parametrize("lo,hi", LIMITS)
def test_decoding_inverts_the_plane_of_stream_maps(fmt, lo, hi):
    codes = np.arange(MAXCODE[fmt] + 1, dtype=DTYPE[fmt]).reshape(1, -1)
    assert np.array_equal(plane_ref(decode_ref(codes, fmt, lo, hi), fmt, lo, hi), codes)


def test_a_nan_decodes_to_the_far_limit():
    v = np.array([[np.nan, -50.0, 50.0, 1.5, np.inf, -np.inf]], f32)
    for lo, hi in ((-12.0, 7.0), (7.0, -12.0)):
        assert np.array_equal(decode_ref(v, "f32", lo, hi), np.array([[7.0, -12.0, 7.0, 1.5, 7.0, -12.0]], f32))


def test_between_equal_backgrounds_fill_1_takes_pixels_from_the_right():
    """a near pole on a flat wall leaves a run whose two sides tie: B = R, and the mirror columns lie right of the run"""
    W = 24
    d = np.full((1, W), 2.0, f32)
    d[0, 10:13] = -3.0  # lands on 7 .. 9; the wall's 0 .. 9 land on 2 .. 11 and its 13 on 15: the runs are 0 .. 1 and 12 .. 14
    img = scene_image(1, W)
    for fill in (0, 1):
        img_r, disp_r, holes, n = eye_ref(img, d, fill, 0.0)
        assert list(np.flatnonzero(holes[0])) == [0, 1, 12, 13, 14] and n["background_ties"] == 1 and (disp_r[0, 12:15] == 2.0).all()
        want = [15, 15, 15] if fill == 0 else [18, 17, 16]
        assert np.array_equal(img_r[0, 12:15], img_r[0, want]), fill


# ----------------------------------------------------------------------------- the two tools
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_take_depth_input_option(tmp_path):
    from stm_amd import video
    one, stack = str(tmp_path / "one.npy"), str(tmp_path / "stack.npy")
    np.save(one, np.zeros((4, 6), np.uint16))
    np.save(stack, np.zeros((2, 4, 6), np.float32))
    argv = ["x", "--depth-input", one, "12", "-3.5", "--cut"]
    planes, setting = video.take_depth_input_option(argv)
    assert planes.shape == (4, 6) and setting == ("u16", 12.0, -3.5, 0, 0.0) and argv == ["x", "--cut"]
    argv = ["--depth-input", stack, "0", "16", "1", "0.5", "y"]
    planes, setting = video.take_depth_input_option(argv, stack=True)
    assert planes.shape == (2, 4, 6) and setting == ("f32", 0.0, 16.0, 1, 0.5) and argv == ["y"]
    assert video.take_depth_input_option(["x"]) is None
    bad64 = str(tmp_path / "f64.npy")
    np.save(bad64, np.zeros((4, 6)))
    for bad in (["--depth-input"], ["--depth-input", one], ["--depth-input", one, "0"], ["--depth-input", one, "1", "1"],
                ["--depth-input", one, "nan", "1"], ["--depth-input", one, "0", "5000"], ["--depth-input", one, "0", "16", "1"],
                ["--depth-input", one, "0", "16", "2", "0.5"], ["--depth-input", one, "0", "16", "1", "-1"],
                ["--depth-input", stack, "0", "16"], ["--depth-input", bad64, "0", "16"],
                ["--depth-input", str(tmp_path / "missing.npy"), "0", "16"], ["--depth-input", one, "x", "16"]):
        with pytest.raises((ValueError, IndexError)):
            video.take_depth_input_option(list(bad))


def test_the_tools_refuse_a_malformed_depth_input_option(tmp_path, capsys):
    one, stack = str(tmp_path / "one.npy"), str(tmp_path / "stack.npy")
    np.save(one, np.zeros((4, 6), np.uint8))
    np.save(stack, np.zeros((2, 4, 6), np.uint8))
    vid, img = _tool("stm_video"), _tool("stm_image")
    for tail in (["--depth-input"], ["--depth-input", stack, "3", "3"], ["--depth-input", one, "0", "16"], ["--depth-input", stack, "0", "16", "1"],
                 ["--depth-input", stack, "0", "16", "--packing", "1", "0", "0", "0"], ["--subpixel", "--depth-input", stack, "0", "16"]):
        assert vid.main(["stm_video"] + ["x"] * 16 + tail) == -1, tail
        assert "--depth-input PLANES.npy" in capsys.readouterr().out
    for tail in (["--depth-input"], ["--depth-input", one, "3", "3"], ["--depth-input", stack, "0", "16"], ["--depth-input", one, "0", "16", "7", "1"],
                 ["--depth-input", one, "0", "16", "--align", "0", "0", "0"], ["--interp", "--depth-input", one, "0", "16"]):
        assert img.main(["stm_image"] + ["x"] * 17 + tail) == -1, tail
        assert "--depth-input PLANE.npy" in capsys.readouterr().out
