"""Depth budget control (stm_set_depth, stm_set_depth_auto, stm_depth_fit): the numpy statement of the definitions in
include/stm_hip.h that the GPU tests (test_gpu_depth.py) compare against bit for bit -- tied to the oracle chain's views and to
test_lens_ref's mode 3 where gain = 1 and conv = 0 make them the same thing -- the disparity a fronto-parallel scene is displayed
with, and the fit's known answers.  No GPU."""
import numpy as np
import pytest

from test_lens_ref import (blend2, chain_views, combine4, frame_chain, lens_phase_ref, lens_pick_ref, render_chain, render_lens_ref,
                           sample_grid, sample_shift_ref, _small_frame)
from test_linwarp_ref import LINEAR_WARP

f32 = np.float32
f64 = np.float64


# ----------------------------------------------------------------------------- the sample rule
def view_shift(v, N):
    """the position of the discrete view v as the reference evaluates it (d_io.cu:189): in double, narrowed"""
    return f32(1.0 - (1.0 * float(f32(v))) / (float(f32(N)) - 1.0))


def depth_map_ref(s, xs, gain, conv, Win):
    """(s2, cx) of a sample for the view position s at the sampling position xs (float32 arrays of one shape): one operation per line"""
    with np.errstate(all="ignore"):
        t = s.astype(f64) - 0.5
        u = f64(f32(gain)) * t
        s2 = (0.5 + u).astype(f32)
        u = f64(f32(conv)) * t
        off = u.astype(f32)
        cx = (xs + off).astype(f32)
        cx = np.fmin(np.fmax(cx, f32(0)), f32(Win - 1))
    return s2, cx


def depth_sample_ref(ch, s, xs, Y0, Y1, wy, c, gain, conv, linear):
    """channel c of the sample for the view position s ([Ho][Wo]) at (xs, row taps Y0 / Y1 / wy): fast_bilinear_interp's combination
    of the four neighbours of (cx, ys), each the renderer's general form at shift s2 (test_lens_ref.sample_shift_ref)"""
    W = ch["L"].shape[1]
    s2, cx = depth_map_ref(s, xs, gain, conv, W)
    X0 = np.floor(cx).astype(np.int64)
    X1 = np.minimum(X0 + 1, W - 1)
    wx = (cx - X0.astype(f32)).astype(f32)
    return combine4(sample_shift_ref(ch, Y0, X0, s2, c, linear), sample_shift_ref(ch, Y0, X1, s2, c, linear),
                    sample_shift_ref(ch, Y1, X0, s2, c, linear), sample_shift_ref(ch, Y1, X1, s2, c, linear), wx, wy)


def depth_view_ref(ch, s, gain, conv, linear):
    """the whole view for the position s, sampled on the input grid (xs = x, ys = y): [H][W][3]"""
    H, W, _ = ch["L"].shape
    Y = np.broadcast_to(np.arange(H)[:, None], (H, W))
    xs = np.broadcast_to(np.arange(W, dtype=f32)[None, :], (H, W))
    sa = np.full((H, W), s, f32)
    return np.stack([depth_sample_ref(ch, sa, xs, Y, Y, np.zeros((H, 1), f32), c, gain, conv, linear) for c in range(3)], axis=-1)


def mux_views_ref(N, angle, elem_sz, Ho, Wo):
    """v[ty][tx][c]: the view mux_multiview_kernel_2 shows in byte c of output pixel (tx, ty) (d_mux_multiview.cu:38-84)"""
    a = f32(f32(angle) * f32(3.1415926535))
    yi = f32(float(f32(N)) / np.tan(float(a) / 180.0) / float(f32(elem_sz)))
    ymod = int(np.floor(float(yi) + 0.5))
    inv_y = f32(1) / yi
    ty = np.arange(Ho)
    off = ((((ty % ymod).astype(f32) + f32(1)) * f32(N)).astype(f32) * inv_y).astype(f32).astype(np.int64)
    r = (3 * np.arange(Wo)[None, :] + off[:, None]) % N
    return (r[..., None] + (2 - np.arange(3))[None, None, :]) % N


def render_depth_ref(ch, N, lens, linear, Ho, Wo, gain, conv, angle=18.43, elem_sz=3):
    """The frame's render with the depth budget (gain, conv) from a render_chain; lens = None (the reference's view assignment) or
    (mode, pitch, slope, centre).  Returns [Ho][Wo][3]."""
    H, W, _ = ch["L"].shape
    (x0, _, wx), (y0, y1, wy) = sample_grid(Ho, Wo, H, W)
    xs = np.broadcast_to((x0.astype(f32) + wx).astype(f32)[None, :], (Ho, Wo))  # floor + fraction: the sampling position, exactly
    Y0, Y1 = np.broadcast_to(y0[:, None], (Ho, Wo)), np.broadcast_to(y1[:, None], (Ho, Wo))
    wy = wy[:, None]
    table = np.array([view_shift(v, N) for v in range(N)], f32)
    mode = 0 if lens is None else lens[0]
    v = w = shift = None
    if mode == 0:
        v = mux_views_ref(N, angle, elem_sz, Ho, Wo)
    else:
        v, w, shift = lens_pick_ref(lens_phase_ref(Ho, Wo, *lens[1:]), N, mode)
    out = np.zeros((Ho, Wo, 3), np.uint8)
    for c in range(3):
        if mode == 3:
            out[..., c] = depth_sample_ref(ch, shift[..., c], xs, Y0, Y1, wy, c, gain, conv, linear)
            continue
        A = depth_sample_ref(ch, table[v[..., c]], xs, Y0, Y1, wy, c, gain, conv, linear)
        if mode == 2:
            B = depth_sample_ref(ch, table[v[..., c] + 1], xs, Y0, Y1, wy, c, gain, conv, linear)
            A = blend2(A, B, w[..., c])
        out[..., c] = A
    return out


# ----------------------------------------------------------------------------- the measurement
def depth_bins_ref(d):
    with np.errstate(all="ignore"):
        v = (np.asarray(d, f32) * f32(4)).astype(f32)
        v = np.fmin(np.fmax(v, f32(-2048)), f32(2047))
        return np.floor((v + f32(0.5)).astype(f32)).astype(np.int64) + 2048


def depth_range_ref(dl, dr, clip_permille):
    """(d_lo, d_hi) as float32: the clipped range of both maps on the quarter-pixel histogram"""
    hist = np.bincount(np.concatenate([depth_bins_ref(dl).ravel(), depth_bins_ref(dr).ravel()]), minlength=4096)
    n = int(hist.sum())
    k = n * int(clip_permille) // 1000
    cum = np.cumsum(hist)
    suf = np.cumsum(hist[::-1])[::-1]
    lo = int(np.argmax(cum > k))
    hi = int(np.nonzero(suf > k)[0].max())
    return f32(f32(lo - 2048) * f32(0.25)), f32(f32(hi - 2048) * f32(0.25)), lo, hi


def depth_fit_ref(dl, dr, disp_lo, disp_hi, max_gain, clip_permille, rate, state):
    """stm_depth_fit: the new state (float32 [4]) from the maps and the old one; the fit in double, one operation per line"""
    d_lo, d_hi, _, _ = depth_range_ref(dl, dr, clip_permille)
    disp_lo, disp_hi, max_gain, rate = float(f32(disp_lo)), float(f32(disp_hi)), float(f32(max_gain)), float(f32(rate))
    span = float(d_hi) - float(d_lo)
    budget = disp_hi - disp_lo
    g = budget / span if span > 0 else max_gain
    g = min(g, max_gain)
    a = g * float(d_hi)
    a = a - disp_hi
    b = g * float(d_lo)
    b = b - disp_lo
    c = min(max(0.0, a), b)
    st = np.array(state, f32)
    if st[0] == 0:
        return np.array([1, g, c, 0], f64).astype(f32)
    for i, value in ((1, g), (2, c)):
        old = float(st[i])
        t = value - old
        t = rate * t
        st[i] = f32(old + t)
    return st


# ----------------------------------------------------------------------------- tie to existing code
@pytest.mark.parametrize("extra", [0, LINEAR_WARP], ids=["truncating", "linear"])
def test_gain_1_conv_0_interior_views_are_the_chains(orc, extra):
    """the statement's views 1 .. N - 2 at gain = 1, conv = 0 are the oracle chain's; the two end views are warps, not the images"""
    sbs, p, H, W = _small_frame()
    ch = frame_chain(orc, sbs, p, extra)
    for N in (5, 8):
        views = chain_views(orc, ch, N, bool(extra))
        for v in range(1, N - 1):
            assert np.array_equal(depth_view_ref(ch, view_shift(v, N), 1.0, 0.0, bool(extra)), views[v][..., :3]), (N, v)
        assert view_shift(0, N) == 1 and view_shift(N - 1, N) == 0
    assert not np.array_equal(depth_view_ref(ch, f32(1), 1.0, 0.0, bool(extra)), ch["R"][..., :3])


@pytest.mark.parametrize("extra", [0, LINEAR_WARP], ids=["truncating", "linear"])
def test_lens_mode_3_with_gain_1_conv_0_is_todays_mode_3(orc, extra):
    sbs, p, H, W = _small_frame()
    ch = frame_chain(orc, sbs, p, extra)
    lens = (3, 7.37, 0.86, 0.3)
    for Ho, Wo in ((H, W), (50, 81)):
        assert np.array_equal(render_depth_ref(ch, 8, lens, bool(extra), Ho, Wo, 1.0, 0.0), render_lens_ref(orc, ch, 8, lens, bool(extra), Ho, Wo))
    assert not np.array_equal(render_depth_ref(ch, 8, lens, False, H, W, 0.5, 0.0), render_lens_ref(orc, ch, 8, lens, False, H, W))


def test_the_references_view_assignment(orc):
    """mux_views_ref is the oracle's interlacer: every view resampled (sample_grid, combine4), then picked per byte"""
    H, W, Ho, Wo = 6, 9, 11, 13
    (x0, x1, wx), (y0, y1, wy) = sample_grid(Ho, Wo, H, W)
    for N in (8, 5):
        rng = np.random.RandomState(N)
        views = [rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(N)]
        res = np.stack([np.stack([combine4(v[y0[:, None], x0[None, :], c], v[y0[:, None], x1[None, :], c], v[y1[:, None], x0[None, :], c],
                                           v[y1[:, None], x1[None, :], c], wx[None, :], wy[:, None]) for c in range(3)], axis=-1) for v in views])
        yy, xx, cc = np.meshgrid(np.arange(Ho), np.arange(Wo), np.arange(3), indexing="ij")
        assert np.array_equal(orc.mux_multiview(views, 18.43, Ho, Wo), res[mux_views_ref(N, 18.43, 3, Ho, Wo), yy, xx, cc])


# ----------------------------------------------------------------------------- displayed disparity
def test_fronto_parallel_pair_is_displayed_with_gain_delta_minus_conv(orc):
    """R(x) = L(x - 8), both maps 8, truncating warps, gain 0.5, conv 2: the end view s = 0 is L(x - 3), the end view s = 1 is
    L(x - 5) -- their difference is gain * 8 - conv = 2.  Compared at least 16 pixels from the border where the chain's planes, at
    the neighbour the sample is taken from, have both masks 1 and blend weight 0."""
    H, W, m = 128, 128, 16
    rng = np.random.RandomState(5)
    L = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    R = np.roll(L, 8, axis=1)
    d = np.full((H, W), 8, f32)
    ch = render_chain(orc, L, R, d, d.copy())
    good = (ch["ml"] == 1) & (ch["mr"] == 1) & (ch["tm"] == 0)
    total = 0
    for s, shown, off in ((f32(0), 3, -1), (f32(1), 5, 1)):
        got = depth_view_ref(ch, s, 0.5, 2.0, False)
        want = np.roll(L, shown, axis=1)
        ok = np.roll(good, -off, axis=1)[m:-m, m:-m]  # the sample of pixel x is taken at x + off
        assert ok.sum() * 2 >= H * W, ok.sum()
        assert np.array_equal(got[m:-m, m:-m][ok], want[m:-m, m:-m][ok]), float(s)
        total += ok.sum()
    assert total > 0


# ----------------------------------------------------------------------------- the fit's known answers
def _fit(dl, dr, lo, hi, mg=1.0, clip=0, rate=1.0, state=(0, 0, 0, 0)):
    return depth_fit_ref(np.asarray(dl, f32), np.asarray(dr, f32), lo, hi, mg, clip, rate, state)


def test_fit_known_answers():
    half = np.array([[-16.0] * 8, [8.0] * 8], f32)
    st = _fit(half, half, -4, 4)
    assert st.tolist() == [1.0, float(f32(1.0 / 3.0)), float(f32(-4.0 / 3.0)), 0.0]
    inside = np.array([[-2.0, 0.0, 3.0, 1.5]], f32)
    assert _fit(inside, inside, -4, 4).tolist() == [1.0, 1.0, 0.0, 0.0]
    sym = np.array([[-2.0, 0.0, 2.0, 1.5]], f32)
    assert _fit(sym, sym, -4, 4, mg=3.0).tolist() == [1.0, 2.0, 0.0, 0.0]  # budget / span = 2, below max_gain: the range fills the budget
    assert _fit(inside, inside, -4, 4, mg=2.0).tolist() == [1.0, float(f32(1.6)), float(f32(1.6 * 3.0 - 4.0)), 0.0]  # [-3.2, 4.8] -> conv 0.8
    flat = np.full((3, 5), 2.25, f32)
    assert _fit(flat, flat, -4, 4, mg=3.0).tolist() == [1.0, 3.0, float(f32(3.0 * 2.25 - 4.0)), 0.0]  # span 0 -> max_gain


def test_histogram_edges():
    assert depth_bins_ref(np.array([np.nan], f32))[0] == 0
    assert depth_bins_ref(np.array([-np.inf, -1e9, -513.0, -512.0], f32)).tolist() == [0, 0, 0, 0]
    assert depth_bins_ref(np.array([np.inf, 1e9, 512.0, 511.75], f32)).tolist() == [4095, 4095, 4095, 4095]
    assert depth_bins_ref(np.array([0.0, 0.125, 0.124, -0.125, -0.126, 0.25], f32)).tolist() == [2048, 2049, 2048, 2048, 2047, 2049]
    nan = np.array([[np.nan, 1.0]], f32)
    d_lo, d_hi, lo, hi = depth_range_ref(nan, nan, 0)
    assert (lo, hi) == (0, 2052) and d_lo == -512 and d_hi == 1


def test_clip_499_keeps_lo_below_hi():
    rng = np.random.RandomState(3)
    for shape in ((1, 1), (3, 5), (7, 9)):
        a = (rng.randint(-40, 40, size=shape) * 0.25).astype(f32)
        b = (rng.randint(-40, 40, size=shape) * 0.25).astype(f32)
        _, _, lo, hi = depth_range_ref(a, b, 499)
        assert lo <= hi
    two = np.array([[1.0]], f32), np.array([[5.0]], f32)
    assert depth_range_ref(*two, 499)[2:] == (2052, 2068)  # n = 2, k = 0: nothing clipped
    many = np.concatenate([np.full(10, -3.0, f32), np.full(980, 1.0, f32), np.full(10, 6.0, f32)])[None, :]
    assert depth_range_ref(many, many, 20)[:2] == (f32(1), f32(1))   # 1 % at either end lies below the 2 % clip
    assert depth_range_ref(many, many, 9)[:2] == (f32(-3), f32(6))


def test_rate_recursion_over_four_frames():
    maps = [np.full((2, 4), v, f32) for v in (8.0, 16.0, 16.0, 2.0)]
    st = np.zeros(4, f32)
    want_g = None
    for k, mp in enumerate(maps):
        dl = np.concatenate([mp, -mp], axis=1)
        st = depth_fit_ref(dl, dl, -4, 4, 1.0, 0, 0.25, st)
        g = min(8.0 / (2 * float(mp[0, 0])), 1.0)
        want_g = g if k == 0 else float(f32(want_g + 0.25 * (g - want_g)))
        assert st[0] == 1 and st[1] == f32(want_g) and st[2] == 0 and st[3] == 0, k
    assert st.tolist() == [1.0, 0.54296875, 0.0, 0.0]  # 0.5 -> 0.4375 -> 0.390625 -> 0.54296875: fits 0.5, 0.25, 0.25, 1


# ----------------------------------------------------------------------------- the tool's options
def test_stm_video_refuses_malformed_depth_options(capsys):
    """--depth needs two values in range, --depth-auto two or five, and the two exclude each other (usage and -1, nothing read)"""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("stm_video", os.path.join(ROOT, "tools", "stm_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for tail in (["--depth", "1"], ["--depth", "9", "0"], ["--depth", "1", "5000"], ["--depth", "x", "0"], ["--depth-auto", "1"],
                 ["--depth-auto", "2", "1"], ["--depth-auto", "-4", "4", "1", "20"], ["--depth-auto", "-4", "4", "1", "500", "1"],
                 ["--depth-auto", "-4", "4", "0", "20", "1"], ["--depth-auto", "-4", "4", "1", "20", "0"],
                 ["--depth", "1", "0", "--depth-auto", "-4", "4"]):
        assert mod.main(["stm_video"] + ["x"] * 16 + tail) == -1, tail
        assert "--depth GAIN CONV | --depth-auto LO HI" in capsys.readouterr().out
