"""Overlay at a chosen depth (stm_mux_overlay, stm_set_overlay): the numpy statement of the definition in include/stm_hip.h that the
GPU tests (test_gpu_overlay.py) compare against bit for bit -- the shift of every sub-pixel taken from the interlacers' own statements
run on constant views, the position, the sample and the blend line by line -- its known answers, and a scalar restatement.  No GPU."""
import math

import numpy as np
import pytest

from test_depth_ref import view_shift
from test_lens_ref import lens_phase_ref, lens_pick_ref, mux_lens_ref
from test_quilt_ref import quilt_ref, tile_origin, tile_size

f32 = np.float32
ANGLE = 18.43
PANEL = (7.37, 0.86, 0.3)  # pitch, slope, centre


# ----------------------------------------------------------------------------- the definition
def view_coords(Ho, Wo, N, layout=None):
    """(vx, vy, valid), [Ho][Wo] each: the view pixel an output pixel is, and whether it is one.  layout None: the frame itself;
    (1, tiles_x, tiles_y, order): a tile's pixel (u, w), false on the remainder pixels that belong to no tile"""
    if layout is None:
        vy, vx = np.meshgrid(np.arange(Ho, dtype=np.int64), np.arange(Wo, dtype=np.int64), indexing="ij")
        return vx, vy, np.ones((Ho, Wo), bool)
    _, tiles_x, tiles_y, order = layout[:4]
    tw, th = tile_size(tiles_x, tiles_y, Ho, Wo)
    vx, vy, valid = np.zeros((Ho, Wo), np.int64), np.zeros((Ho, Wo), np.int64), np.zeros((Ho, Wo), bool)
    for v in range(N):
        left, top = tile_origin(v, N, tiles_x, tiles_y, order, Ho, Wo)
        vx[top:top + th, left:left + tw] = np.arange(tw)[None, :]
        vy[top:top + th, left:left + tw] = np.arange(th)[:, None]
        valid[top:top + th, left:left + tw] = True
    return vx, vy, valid


def discrete_shift(v, N):
    """s of a discrete view index (any integer array): (float)(1.0 - (double)(float)v / ((double)(float)N - 1.0))"""
    return (1.0 - v.astype(f32).astype(np.float64) / (float(f32(N)) - 1.0)).astype(f32)


def subpixel_shift_ref(orc, Ho, Wo, N, elem_sz=3, angle=ANGLE, lens=None, layout=None):
    """shift[y][x][c], float32: the camera position byte c of output pixel (x, y) shows (step 1 of the definition).  The discrete view
    indices come from the interlacers' own statements on constant 1 x 1 views (view v filled with v: its sampler returns v exactly):
    the oracle's orc_mux_multiview (the form that multiplies by 1 / y_interval), mux_lens_ref, quilt_ref.  lens = (mode, pitch,
    slope, centre) or None; layout = (1, tiles_x, tiles_y, order) or None.  Remainder pixels of a quilt get NaN."""
    const = [np.full((1, 1, elem_sz), v, np.uint8) for v in range(N)]
    if layout is not None:
        assert lens is None or lens[0] == 0
        _, tiles_x, tiles_y, order = layout[:4]
        v1 = quilt_ref([c + 1 for c in const], tiles_x, tiles_y, order, 0, Ho, Wo).astype(np.int64)  # 0 = no tile
        s = discrete_shift(np.maximum(v1 - 1, 0), N)
        s[v1 == 0] = np.nan
        return s
    if lens is None or lens[0] == 0:
        v = orc.mux_multiview(const, angle, Ho, Wo, variant=2)[..., :3]
        return discrete_shift(v.astype(np.int64), N)
    mode, pitch, slope, centre = lens
    if mode == 1:
        return discrete_shift(mux_lens_ref(const, 1, pitch, slope, centre, Ho, Wo).astype(np.int64), N)
    return lens_pick_ref(lens_phase_ref(Ho, Wo, pitch, slope, centre), N, 3)[2]


def overlay_ref(frame, overlay, x0, y0, disparity, shift, coords=None):
    """stm_mux_overlay: the frame ([Ho][Wo][E] u8) with the overlay ([rows][cols][4] u8, premultiplied) composited at view pixel
    (x0, y0) and the end-to-end disparity; shift = subpixel_shift_ref's, coords = view_coords' (None: layout 0).  A new array."""
    frame, O = np.asarray(frame), np.asarray(overlay).astype(np.int64)
    Ho, Wo, _ = frame.shape
    rows, cols, _ = O.shape
    vx, vy, valid = coords if coords is not None else view_coords(Ho, Wo, 0)
    with np.errstate(invalid="ignore"):
        t = shift.astype(np.float64) - 0.5
        o = float(f32(disparity)) * t
        p = (vx - int(x0)).astype(np.float64)[..., None] - o
        p = p * 256.0
        F = np.floor(np.where(np.isnan(p), 0.0, p)).astype(np.int64)
    q, fr = F >> 8, F & 255
    r = vy - int(y0)
    inside = (valid & (r >= 0) & (r < rows))[..., None] & np.ones(3, bool)
    rr = np.clip(r, 0, rows - 1)[..., None]

    def column(k):  # O[r][k] with a column outside [0, cols) read as 0: [Ho][Wo][3][4]
        ok = (k >= 0) & (k < cols)
        return np.where(ok[..., None], O[rr, np.clip(k, 0, cols - 1)], 0)
    I = (256 - fr)[..., None] * column(q) + fr[..., None] * column(q + 1)
    c = np.arange(3)
    Ic, Ia = I[..., c, c], I[..., 3]
    dst = frame[..., :3].astype(np.int64)
    num = 255 * Ic + (65280 - Ia) * dst + 32640
    assert num.max() < 1 << 26
    out = frame.copy()
    out[..., :3] = np.where(inside, np.minimum(255, num // 65280), dst).astype(np.uint8)
    return out


def overlay_scalar(frame, overlay, x0, y0, disparity, shift, coords):
    """the same lines, one sub-pixel at a time in Python's own arithmetic: the twin that keeps the vectorised statement honest"""
    vx, vy, valid = coords
    out = frame.copy()
    rows, cols, _ = overlay.shape
    d = float(f32(disparity))

    def px(r, k):
        return [int(b) for b in overlay[r, k]] if 0 <= k < cols else [0, 0, 0, 0]
    for y in range(frame.shape[0]):
        for x in range(frame.shape[1]):
            r = int(vy[y, x]) - y0
            if not valid[y, x] or not 0 <= r < rows:
                continue
            for c in range(3):
                F = math.floor(((int(vx[y, x]) - x0) - d * (float(shift[y, x, c]) - 0.5)) * 256.0)
                q, fr = F >> 8, F & 255
                P0, P1 = px(r, q), px(r, q + 1)
                Ic, Ia = (256 - fr) * P0[c] + fr * P1[c], (256 - fr) * P0[3] + fr * P1[3]
                out[y, x, c] = min(255, (255 * Ic + (65280 - Ia) * int(frame[y, x, c]) + 32640) // 65280)
    return out


def random_overlay(seed, rows, cols):
    """a random premultiplied overlay with fully transparent, fully opaque and partial pixels"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(rows, cols, 1))
    kind = rng.randint(0, 4, size=(rows, cols, 1))
    a = np.where(kind == 0, 0, np.where(kind == 1, 255, a))
    colour = (rng.randint(0, 256, size=(rows, cols, 3)) * a + 127) // 255
    return np.concatenate([colour, a], axis=-1).astype(np.uint8)


def _frame(seed, Ho, Wo, E=3):
    return np.random.RandomState(seed).randint(0, 256, size=(Ho, Wo, E)).astype(np.uint8)


GEOMETRIES = [dict(), dict(lens=(1,) + PANEL), dict(lens=(2,) + PANEL), dict(lens=(3,) + PANEL), dict(layout=(1, 4, 2, 0)),
              dict(layout=(1, 2, 4, 3))]


# ----------------------------------------------------------------------------- known answers
def test_the_blend_lines_over_every_dst():
    """what the header says of step 4, checked over all dst"""
    dst = np.arange(256, dtype=np.int64)
    assert np.array_equal((255 * 0 + 65280 * dst + 32640) // 65280, dst)  # I_c = I_3 = 0 leaves dst
    for Ic in range(0, 65281, 7):  # full alpha gives I_c / 256, rounded to nearest, whatever dst
        assert np.array_equal((255 * Ic + 0 * dst + 32640) // 65280, np.full(256, (2 * Ic + 256) // 512))
    for Ia in range(0, 65281, 257):  # premultiplied (I_c <= I_3): the result stays in 0 .. 255 without the min
        for Ic in (0, Ia // 2, Ia):
            v = (255 * Ic + (65280 - Ia) * dst + 32640) // 65280
            assert v.min() >= 0 and v.max() <= 255


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_a_transparent_overlay_is_the_identity(orc, geom):
    Ho, Wo, N = 22, 36, 8
    f = _frame(1, Ho, Wo, 4)
    s = subpixel_shift_ref(orc, Ho, Wo, N, 4, **geom)
    got = overlay_ref(f, np.zeros((5, 9, 4), np.uint8), 3, 4, -6.5, s, view_coords(Ho, Wo, N, geom.get("layout")))
    assert np.array_equal(got, f)


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_opaque_at_disparity_0_reproduces_its_colours(orc, geom):
    Ho, Wo, N = 24, 40, 8
    f = _frame(2, Ho, Wo)
    ov = random_overlay(3, 4, 6)
    ov[..., 3] = 255
    coords = view_coords(Ho, Wo, N, geom.get("layout"))
    got = overlay_ref(f, ov, 2, 1, 0.0, subpixel_shift_ref(orc, Ho, Wo, N, 3, **geom), coords)
    vx, vy, valid = coords
    inside = valid & (vx >= 2) & (vx < 8) & (vy >= 1) & (vy < 5)
    assert inside.sum() == (24 if "layout" not in geom else 24 * 8)
    assert np.array_equal(got[inside], ov[vy[inside] - 1, vx[inside] - 2, :3])
    assert np.array_equal(got[~inside], f[~inside])


def test_quilt_parallax_of_an_opaque_marker(orc):
    """the parallax the feature is for: disparity 14 over N = 8 views puts the marker's left edge at x0 + 7, + 5, ..., - 7 in the
    tiles of views 0 .. 7.  (s is a float: where (s - 0.5) * 14 rounds a hair above the whole number the edge column carries
    255/256 of the marker and the column before it nothing; a hair below, the edge column everything and the one before 1/256.)"""
    Ho, Wo, N, lay = 20, 4 * 30 + 3, 8, (1, 4, 2, 0)
    ov = np.full((3, 5, 4), 255, np.uint8)
    x0, y0 = 12, 2
    got = overlay_ref(np.zeros((Ho, Wo, 3), np.uint8), ov, x0, y0, 14.0, subpixel_shift_ref(orc, Ho, Wo, N, layout=lay), view_coords(Ho, Wo, N, lay))
    for v in range(N):
        left, top = tile_origin(v, N, 4, 2, 0, Ho, Wo)
        tile = got[top + y0, left:left + 30, 0].astype(int)
        edge = x0 + 7 - 2 * v
        assert int(np.argmax(tile >= 128)) == edge, (v, tile)
        assert tile[edge] >= 254 and tile[edge - 1] <= 1 and (tile[:edge - 1] == 0).all(), (v, tile)
        assert (tile[edge + 1:edge + 5] == 255).all() and tile[edge + 5] <= 1 and (tile[edge + 6:] == 0).all(), (v, tile)
    assert (got[:, 120:] == 0).all()  # the remainder columns are never touched


def test_a_half_pixel_shift_fades_the_edge_columns_by_half():
    Ho, Wo = 3, 12
    f = _frame(5, Ho, Wo)
    ov = np.zeros((1, 4, 4), np.uint8)
    ov[0, :] = (200, 100, 50, 255)
    s = np.ones((Ho, Wo, 3), f32)  # (s - 0.5) * 1 = half a pixel to the right
    got = overlay_ref(f, ov, 4, 1, 1.0, s)
    col = np.array([200, 100, 50])
    for x in (4, 8):  # I = 128 * P for colour and alpha alike
        want = (255 * 128 * col + (65280 - 128 * 255) * f[1, x].astype(np.int64) + 32640) // 65280
        assert np.array_equal(got[1, x], want)
    assert np.array_equal(got[1, 5:8], np.broadcast_to(col, (3, 3)))
    untouched = np.ones((Ho, Wo), bool)
    untouched[1, 4:9] = False
    assert np.array_equal(got[untouched], f[untouched])


@pytest.mark.parametrize("x0,y0", [(-3, 2), (30, 2), (5, -2), (5, 17), (-3, -2), (30, 17)])
def test_parts_outside_the_view_are_clipped(orc, x0, y0):
    Ho, Wo, N = 20, 36, 8
    f = _frame(6, Ho, Wo)
    ov = random_overlay(7, 5, 9)
    s = subpixel_shift_ref(orc, Ho, Wo, N)
    got = overlay_ref(f, ov, x0, y0, 0.0, s)
    # the same overlay cut to the part inside the view, placed where that part starts
    cx0, cy0 = max(x0, 0), max(y0, 0)
    cut = ov[cy0 - y0:min(y0 + 5, Ho) - y0, cx0 - x0:min(x0 + 9, Wo) - x0]
    assert cut.size and np.array_equal(got, overlay_ref(f, cut, cx0, cy0, 0.0, s))
    assert np.array_equal(got, overlay_scalar(f, ov, x0, y0, 0.0, s, view_coords(Ho, Wo, N)))


@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("disparity", [2.5, -13.75, 600.0])
def test_the_scalar_twin_agrees_also_beyond_the_overlays_width(orc, geom, disparity):
    """3 x 5 pixels shifted by up to 300: wherever the overlay lands, or lands outside, the two statements agree"""
    Ho, Wo, N = 16, 26, 8
    f = _frame(8, Ho, Wo, 4)
    ov = random_overlay(9, 3, 5)
    coords = view_coords(Ho, Wo, N, geom.get("layout"))
    s = subpixel_shift_ref(orc, Ho, Wo, N, 4, **geom)
    got = overlay_ref(f, ov, 1, 1, disparity, s, coords)
    assert np.array_equal(got, overlay_scalar(f, ov, 1, 1, disparity, s, coords))
    assert np.array_equal(got[..., 3], f[..., 3])  # bytes 3 .. are never written
    if abs(disparity) < 100:
        assert not np.array_equal(got, f)


def test_the_shift_follows_the_pixel_size_through_the_interlacers_period(orc):
    """the reference's y_interval divides by elem_sz, so a 4-byte frame is interlaced differently: the statement follows the oracle"""
    assert not np.array_equal(subpixel_shift_ref(orc, 16, 16, 8, 3), subpixel_shift_ref(orc, 16, 16, 8, 4))
    s = subpixel_shift_ref(orc, 16, 16, 8, 3)
    assert set(np.unique(s)) == set(float(view_shift(v, 8)) for v in range(8))


def test_premultiply():
    import stm_amd
    from stm_amd import video
    del stm_amd
    a = np.array([[[255, 0, 10, 128], [1, 2, 3, 0], [9, 8, 7, 255], [255, 255, 255, 1]]], np.uint8)
    p = video.premultiply(a)
    assert p.tolist() == [[[128, 0, 5, 128], [0, 0, 0, 0], [9, 8, 7, 255], [1, 1, 1, 1]]]
    assert (p[..., :3] <= p[..., 3:]).all()


def test_tools_refuse_a_malformed_overlay_option(capsys, tmp_path):
    """--overlay needs its file and three numbers, and the file must hold uint8 [rows][cols][4] (usage and -1, nothing run)"""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("stm_video", os.path.join(ROOT, "tools", "stm_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bad = tmp_path / "bad.npy"
    np.save(bad, np.zeros((4, 4, 3), np.uint8))
    good = tmp_path / "good.npy"
    np.save(good, np.zeros((4, 4, 4), np.uint8))
    for tail in (["--overlay", str(good), "1", "2"], ["--overlay", str(bad), "1", "2", "3.5"], ["--overlay", str(good), "1", "x", "3.5"],
                 ["--overlay", str(tmp_path / "missing.npy"), "1", "2", "3.5"]):
        assert mod.main(["stm_video"] + ["x"] * 16 + tail) == -1, tail
        assert "--overlay FILE.npy X0 Y0 DISPARITY" in capsys.readouterr().out
