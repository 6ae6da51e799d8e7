"""Quilt output (stm_set_layout, stm_quilt_multiview): the numpy statement of the definition in include/stm_hip.h that the GPU tests
(test_gpu_quilt.py) compare against bit for bit -- the tile geometry, the reference's four-neighbour sampler per tile (filter 0), the
exact area average (filter 1) -- its known answers, and the area average against an independent statement in exact fractions.
No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from test_depth_ref import depth_sample_ref, depth_view_ref, view_shift
from test_lens_ref import chain_views, combine4, random_views, sample_grid

f32 = np.float32


# ----------------------------------------------------------------------------- the definition
def tile_size(tiles_x, tiles_y, Ho, Wo):
    return Wo // tiles_x, Ho // tiles_y


def tile_origin(v, N, tiles_x, tiles_y, order, Ho, Wo):
    """(left, top) of the tile view v goes to"""
    tw, th = tile_size(tiles_x, tiles_y, Ho, Wo)
    k = N - 1 - v if order & 2 else v
    i, j = k % tiles_x, k // tiles_x
    return i * tw, (Ho - (j + 1) * th if order & 1 else j * th)


def area_weights(t, n):
    """w[u][x]: the overlap of tile interval u (of t) with view interval x (of n) in units of 1 / t of a view pixel; int64 [t][n]"""
    u = np.arange(t, dtype=np.int64)[:, None]
    x = np.arange(n, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((u + 1) * n, (x + 1) * t) - np.maximum(u * n, x * t))


def resample_tile(view, tw, th, filter):
    """one view ([Hin][Win][>= 3] u8) as a th x tw tile: [th][tw][3]"""
    view = np.asarray(view)[..., :3]
    Hin, Win, _ = view.shape
    if filter == 0:
        (x0, x1, wx), (y0, y1, wy) = sample_grid(th, tw, Hin, Win)
        return np.stack([combine4(view[y0[:, None], x0[None, :], c], view[y0[:, None], x1[None, :], c], view[y1[:, None], x0[None, :], c],
                                  view[y1[:, None], x1[None, :], c], wx[None, :], wy[:, None]) for c in range(3)], axis=-1)
    assert filter == 1
    wy, wx = area_weights(th, Hin), area_weights(tw, Win)
    den = Win * Hin
    acc = np.einsum("wy,yxc,ux->wuc", wy, view.astype(np.int64), wx)
    return ((acc + den // 2) // den).astype(np.uint8)


def place_tiles(tiles, tiles_x, tiles_y, order, Ho, Wo):
    """tiles[v] = [th][tw][3] -> the quilt [Ho][Wo][3]; pixels of no tile are 0"""
    N = len(tiles)
    assert tiles_x * tiles_y == N
    tw, th = tile_size(tiles_x, tiles_y, Ho, Wo)
    assert tw >= 1 and th >= 1
    out = np.zeros((Ho, Wo, 3), np.uint8)
    for v in range(N):
        left, top = tile_origin(v, N, tiles_x, tiles_y, order, Ho, Wo)
        assert tiles[v].shape == (th, tw, 3)
        out[top:top + th, left:left + tw] = tiles[v]
    return out


def quilt_ref(V, tiles_x, tiles_y, order, filter, Ho, Wo):
    """stm_quilt_multiview: V = the N views ([N][Hin][Win][>= 3] u8, or a list), V[0] = the right image.  Returns [Ho][Wo][3]."""
    tw, th = tile_size(tiles_x, tiles_y, Ho, Wo)
    return place_tiles([resample_tile(v, tw, th, filter) for v in V], tiles_x, tiles_y, order, Ho, Wo)


def render_views_ref(orc, ch, N, linear, depth=None):
    """V of a frame from a render_chain: the frame's views (depth None), or the depth budget's at depth = (gain, conv)"""
    if depth is None:
        return [np.asarray(v)[..., :3] for v in chain_views(orc, ch, N, linear)]
    return [depth_view_ref(ch, view_shift(v, N), depth[0], depth[1], linear) for v in range(N)]


def render_quilt_ref(orc, ch, N, tiles_x, tiles_y, order, filter, Ho, Wo, linear=False, depth=None):
    """The frame's output under layout 1 from a render_chain; depth = None (mode 0) or (gain, conv).  Filter 1 averages the views V;
    filter 0 takes the renderer's own sample at the fractional position: the four-neighbour combination of view v's samples without
    a depth budget, stm_set_depth's sample rule at (xs, ys) with one."""
    if filter == 1 or depth is None:
        return quilt_ref(render_views_ref(orc, ch, N, linear, depth), tiles_x, tiles_y, order, filter, Ho, Wo)
    H, W, _ = ch["L"].shape
    tw, th = tile_size(tiles_x, tiles_y, Ho, Wo)
    (x0, _, wx), (y0, y1, wy) = sample_grid(th, tw, H, W)
    xs = np.broadcast_to((x0.astype(f32) + wx).astype(f32)[None, :], (th, tw))
    Y0, Y1 = np.broadcast_to(y0[:, None], (th, tw)), np.broadcast_to(y1[:, None], (th, tw))
    tiles = []
    for v in range(N):
        s = np.full((th, tw), view_shift(v, N), f32)
        tiles.append(np.stack([depth_sample_ref(ch, s, xs, Y0, Y1, wy[:, None], c, depth[0], depth[1], linear) for c in range(3)], axis=-1))
    return place_tiles(tiles, tiles_x, tiles_y, order, Ho, Wo)


# ----------------------------------------------------------------------------- an independent statement of filter 1
def area_mean_fractions(view, tw, th):
    """the mean of the view over each tile pixel's footprint in exact fractions, rounded half up: [th][tw][3]"""
    Hin, Win, _ = view.shape

    def overlaps(u, t, n):
        a, b = Fraction(u * n, t), Fraction((u + 1) * n, t)
        return [(x, min(b, Fraction(x + 1)) - max(a, Fraction(x))) for x in range(n) if min(b, Fraction(x + 1)) > max(a, Fraction(x))]
    out = np.zeros((th, tw, 3), np.uint8)
    for w in range(th):
        oy = overlaps(w, th, Hin)
        for u in range(tw):
            ox = overlaps(u, tw, Win)
            area = sum(l for _, l in oy) * sum(l for _, l in ox)
            assert area == Fraction(Hin, th) * Fraction(Win, tw)
            for c in range(3):
                mean = sum(ly * lx * int(view[y, x, c]) for y, ly in oy for x, lx in ox) / area
                out[w, u, c] = (mean + Fraction(1, 2)).__floor__()
    return out


# ----------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("t,n", [(1, 1), (1, 7), (7, 1), (3, 7), (7, 3), (4, 64), (257, 257), (257, 7), (35, 64), (420, 1920)])
def test_weights_of_every_column_sum_to_the_views_size(t, n):
    w = area_weights(t, n)
    assert (w.sum(axis=1) == n).all() and (w.sum(axis=0) == t).all()
    for u in (0, t // 2, t - 1):  # non-zero exactly on x = u n / t .. ((u + 1) n - 1) / t
        nz = np.nonzero(w[u])[0]
        assert nz[0] == (u * n) // t and nz[-1] == ((u + 1) * n - 1) // t and len(nz) == nz[-1] - nz[0] + 1
    if t >= n:
        assert (np.count_nonzero(w, axis=1) <= 2).all()  # up-scaling: a tile pixel overlaps at most two view pixels


@pytest.mark.parametrize("filter", [0, 1])
def test_tiles_of_the_views_own_size_return_the_views(filter):
    """Win = 64 is a power of two, so (u / tw) * Win is exact in float; Hin = 8 likewise"""
    N, H, W = 6, 8, 64
    V = random_views(11, N, H, W)
    out = quilt_ref(V, 3, 2, 0, filter, 2 * H, 3 * W)
    for v in range(N):
        i, j = v % 3, v // 3
        assert np.array_equal(out[j * H:(j + 1) * H, i * W:(i + 1) * W], V[v])


def test_integer_ratio_is_the_plain_mean_rounded_half_up():
    N, H, W = 2, 6, 8
    V = random_views(12, N, H, W)
    out = quilt_ref(V, 2, 1, 0, 1, H // 2, 2 * (W // 4))  # footprints 2 rows x 4 columns
    for v in range(N):
        blocks = V[v].astype(np.int64).reshape(H // 2, 2, W // 4, 4, 3).sum(axis=(1, 3))
        assert np.array_equal(out[:, v * 2:(v + 1) * 2], ((blocks + 4) // 8).astype(np.uint8))
    one = np.zeros((1, 2, 3), np.uint8)
    one[0, :, 0], one[0, :, 1], one[0, :, 2] = (0, 1), (2, 3), (255, 254)  # means 0.5, 2.5, 254.5
    assert resample_tile(one, 1, 1, 1)[0, 0].tolist() == [1, 3, 255]


@pytest.mark.parametrize("filter", [0, 1])
def test_constant_views_give_constant_tiles(filter):
    N = 4
    V = [np.full((5, 9, 3), 10 * v + 255 - 40, np.uint8) for v in range(N)]
    for Ho, Wo in ((10, 18), (7, 11), (23, 40)):
        out = quilt_ref(V, 2, 2, 0, filter, Ho, Wo)
        tw, th = tile_size(2, 2, Ho, Wo)
        for v in range(N):
            left, top = tile_origin(v, N, 2, 2, 0, Ho, Wo)
            assert (out[top:top + th, left:left + tw] == V[v][0, 0, 0]).all(), (Ho, Wo, v)


def test_orders_place_the_end_views():
    """3 x 2 tiles of 2 x 2 pixels in a 5 x 7 frame; view 0 is the right image.  order 0: view 0 top left, view 5 bottom right (of
    the tiles); bit 0 turns the rows over; bit 1 reverses the views"""
    N, Ho, Wo = 6, 5, 7
    V = [np.full((2, 2, 3), 10 * (v + 1), np.uint8) for v in range(N)]
    want = {0: ((0, 0), (4, 2)), 1: ((0, 3), (4, 1)), 2: ((4, 2), (0, 0)), 3: ((4, 1), (0, 3))}  # order: (left, top) of views 0 and 5
    for order, (first, last) in want.items():
        assert tile_origin(0, N, 3, 2, order, Ho, Wo) == first and tile_origin(N - 1, N, 3, 2, order, Ho, Wo) == last, order
        out = quilt_ref(V, 3, 2, order, 1, Ho, Wo)
        assert out[first[1], first[0], 0] == 10 and out[last[1], last[0], 0] == 60
        # remainder: the column at the right always, the row at the bottom (top-down) or at the top (bottom-up)
        assert (out[:, 6] == 0).all()
        assert (out[0 if order & 1 else 4] == 0).all()
        assert (out[1:5, :6] if order & 1 else out[0:4, :6]).min() == 10
        assert sorted(set(out[..., 0].ravel().tolist())) == [0, 10, 20, 30, 40, 50, 60]


@pytest.mark.parametrize("case", [((1, 1), (1, 1)), ((7, 9), (3, 4)), ((3, 4), (7, 9)), ((7, 9), (7, 9)), ((5, 2), (2, 5)), ((6, 9), (4, 6)),
                                  ((7, 9), (1, 1))], ids=str)
def test_area_filter_against_exact_fractions(case):
    (Hin, Win), (th, tw) = case
    view = random_views(Hin * 16 + tw, 1, Hin, Win)[0]
    assert np.array_equal(resample_tile(view, tw, th, 1), area_mean_fractions(view, tw, th))


def test_filter_0_is_the_interlacers_sampler():
    """one tile of the frame's own size samples like mux_multiview_kernel_2: with N identical views the interlaced frame is that view resampled"""
    from conftest import ROOT  # noqa: F401
    H, W, Ho, Wo = 6, 9, 11, 13
    view = random_views(5, 1, H, W)[0]
    (x0, x1, wx), (y0, y1, wy) = sample_grid(Ho, Wo, H, W)
    want = np.stack([combine4(view[y0[:, None], x0[None, :], c], view[y0[:, None], x1[None, :], c], view[y1[:, None], x0[None, :], c],
                              view[y1[:, None], x1[None, :], c], wx[None, :], wy[:, None]) for c in range(3)], axis=-1)
    assert np.array_equal(resample_tile(view, Wo, Ho, 0), want)


def test_frame_views_tie_to_the_chain(orc):
    """filter 1 with tiles of the views' own size returns the frame's views: the chain's without a depth budget, and at gain 1,
    conv 0 the same interior views with warped end views"""
    from test_lens_ref import _small_frame, frame_chain
    sbs, p, H, W = _small_frame()
    ch = frame_chain(orc, sbs, p, 0)
    N = 4
    views = chain_views(orc, ch, N, False)
    out = render_quilt_ref(orc, ch, N, 2, 2, 0, 1, 2 * H, 2 * W)
    outd = render_quilt_ref(orc, ch, N, 2, 2, 0, 1, 2 * H, 2 * W, depth=(1.0, 0.0))
    for v in range(N):
        i, j = v % 2, v // 2
        assert np.array_equal(out[j * H:(j + 1) * H, i * W:(i + 1) * W], views[v][..., :3])
        same = np.array_equal(outd[j * H:(j + 1) * H, i * W:(i + 1) * W], views[v][..., :3])
        assert same == (0 < v < N - 1), v


# ----------------------------------------------------------------------------- the tools' option
def test_tools_refuse_a_malformed_quilt_option(capsys):
    import importlib.util
    import os
    from conftest import ROOT
    for tool, n in (("stm_video", 16), ("stm_image", 17)):
        spec = importlib.util.spec_from_file_location(tool, os.path.join(ROOT, "tools", tool + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        for tail in (["--quilt", "4", "2"], ["--quilt", "4", "2", "0"], ["--quilt", "0", "2", "0", "1"], ["--quilt", "4", "2", "4", "1"],
                     ["--quilt", "4", "2", "0", "2"], ["--quilt", "4", "x", "0", "1"],
                     ["--lens", "1", "8", "1", "0", "--quilt", "4", "2", "0", "1"]):
            assert mod.main([tool] + ["x"] * n + tail) == -1, (tool, tail)
            assert "--quilt TX TY ORDER FILTER" in capsys.readouterr().out
