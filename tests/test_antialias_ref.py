"""View antialiasing (stm_view_prefilter, stm_set_antialias): the numpy statement of the definition in include/stm_hip.h that the GPU
tests (test_gpu_antialias.py) compare against bit for bit -- a scalar form that follows the header line by line, a vectorised form
tied to it pixel by pixel -- its known answers, its edge property, and what it buys on the oracle's own renderer.  No GPU."""
import numpy as np
import pytest

f32 = np.float32


# ----------------------------------------------------------------------------- the definition
def half_width(delta, num_views, strength, max_radius, gain=1.0, conv=0.0):
    """H of one pixel: the per-side extension in 1/16 px"""
    k16 = f32(float(strength) * 8.0 / float(num_views - 1))
    with np.errstate(invalid="ignore", over="ignore"):
        p = f32(gain) * f32(delta)
        e = p - f32(conv)
        a = np.abs(e)
        if not np.isfinite(a):
            return 0
        t = a * k16
        t = min(t, f32(16 * max_radius))  # a finite: t is no NaN
        return int(f32(t) + f32(0.5))


def prefilter_ref(img, disp, num_views, strength, max_radius, gate, gain=1.0, conv=0.0):
    """The scalar statement: img uint8 [H][W][E >= 3] filtered by its own map disp float32 [H][W]; returns uint8 [H][W][3]"""
    img = np.asarray(img, np.uint8)
    disp = np.asarray(disp, f32)
    rows, cols = disp.shape
    out = np.zeros((rows, cols, 3), np.uint8)
    g = f32(gate)
    for y in range(rows):
        for x in range(cols):
            H = half_width(disp[y, x], num_views, strength, max_radius, gain, conv)
            K = (H + 15) >> 4
            T = 16
            acc = [16 * int(img[y, x, c]) for c in range(3)]
            for k in range(1, K + 1):
                w = min(16, H - 16 * (k - 1))
                for j in (x - k, x + k):
                    jc = min(max(j, 0), cols - 1)
                    with np.errstate(invalid="ignore"):
                        used = bool(np.abs(disp[y, jc] - disp[y, x]) <= g)  # false for NaN
                    if used:
                        T += w
                        for c in range(3):
                            acc[c] += w * int(img[y, jc, c])
            for c in range(3):
                out[y, x, c] = (acc[c] + (T >> 1)) // T
    return out


def prefilter_vec(img, disp, num_views, strength, max_radius, gate, gain=1.0, conv=0.0, return_T=False):
    """prefilter_ref, a row of taps at a time (what the GPU tests use on whole frames); return_T: the divisors T [H][W] as well"""
    img = np.asarray(img, np.uint8)
    d = np.asarray(disp, f32)
    rows, cols = d.shape
    k16 = f32(float(strength) * 8.0 / float(num_views - 1))
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(f32(gain) * d - f32(conv))
        fin = np.isfinite(a)
        t = np.minimum(np.where(fin, a, f32(0)) * k16, f32(16 * max_radius)) + f32(0.5)
    H = np.where(fin, t.astype(np.int64), 0)
    K = (H + 15) >> 4
    T = np.full((rows, cols), 16, np.int64)
    acc = 16 * img[..., :3].astype(np.int64)
    xs = np.arange(cols)
    for k in range(1, int(K.max()) + 1 if K.size else 1):
        w = np.where(k <= K, np.minimum(16, H - 16 * (k - 1)), 0)
        for j in (xs - k, xs + k):
            jc = np.clip(j, 0, cols - 1)
            with np.errstate(invalid="ignore"):
                used = np.abs(d[:, jc] - d) <= f32(gate)
            wu = np.where(used, w, 0)
            T += wu
            acc += wu[..., None] * img[:, jc, :3].astype(np.int64)
    out = ((acc + (T >> 1)[..., None]) // T[..., None]).astype(np.uint8)
    return (out, T) if return_T else out


def delta_for_half_width(H, num_views=8):
    """a delta whose H is exactly `H` at strength 1, gain 1, conv 0 and a max_radius that does not clamp it"""
    d = f32(H * (num_views - 1) / 8.0)
    assert half_width(d, num_views, 1.0, 16) == H
    return d


# ----------------------------------------------------------------------------- known answers
ROW = np.array([[10, 20, 30, 40, 50, 60, 70, 80, 90]], np.uint8)


def row_img(vals=ROW):
    return np.stack([vals, 255 - vals, vals // 2], axis=-1).astype(np.uint8)


def test_half_width_zero_copies():
    img = row_img()
    out = prefilter_ref(img, np.zeros((1, 9), f32), 8, 1.0, 8, 1.0)
    assert np.array_equal(out, img)


def test_half_width_8_by_hand():
    """H = 8: K = 1, w_1 = 8, T = 32: (16 c + 8 (l + r) + 16) / 32"""
    d = np.full((1, 9), delta_for_half_width(8), f32)
    out = prefilter_ref(row_img(), d, 8, 1.0, 8, 1.0)
    v = ROW[0].astype(int)
    for x in range(1, 8):
        assert out[0, x, 0] == (16 * v[x] + 8 * (v[x - 1] + v[x + 1]) + 16) // 32
    # clamping at both ends: the tap outside is the end pixel itself
    assert out[0, 0, 0] == (16 * 10 + 8 * (10 + 20) + 16) // 32 == 13
    assert out[0, 8, 0] == (16 * 90 + 8 * (80 + 90) + 16) // 32 == 88
    assert out[0, 4, 0] == 50 and out[0, 4, 1] == 205  # a linear ramp stays put in the interior


def test_half_width_16_and_24_by_hand():
    v = ROW[0].astype(int)
    d = np.full((1, 9), delta_for_half_width(16), f32)
    out = prefilter_ref(row_img(), d, 8, 1.0, 8, 1.0)
    assert out[0, 4, 0] == (16 * (v[3] + v[4] + v[5]) + 24) // 48 == 50  # K = 1, w_1 = 16, T = 48
    assert out[0, 0, 0] == (16 * (10 + 10 + 20) + 24) // 48 == 13
    d = np.full((1, 9), delta_for_half_width(24), f32)
    out = prefilter_ref(row_img(), d, 8, 1.0, 8, 1.0)
    # K = 2, w_1 = 16, w_2 = 8, T = 16 + 32 + 16 = 64
    assert out[0, 4, 0] == (16 * (v[3] + v[4] + v[5]) + 8 * (v[2] + v[6]) + 32) // 64 == 50
    assert out[0, 0, 0] == (16 * (10 + 10 + 20) + 8 * (10 + 30) + 32) // 64 == 15
    assert out[0, 8, 0] == (16 * (80 + 90 + 90) + 8 * (70 + 90) + 32) // 64 == 85
    # max_radius clamps H: radius 1 turns H = 24 into 16
    assert np.array_equal(prefilter_ref(row_img(), d, 8, 1.0, 1, 1.0),
                          prefilter_ref(row_img(), np.full((1, 9), delta_for_half_width(16), f32), 8, 1.0, 8, 1.0))


def test_gate_rejects_a_tap():
    d = np.full((1, 9), delta_for_half_width(16), f32)
    d[0, 5] += f32(3.0)  # pixel 5 lies on another surface
    out = prefilter_ref(row_img(), d, 8, 1.0, 8, 1.0)
    v = ROW[0].astype(int)
    assert out[0, 4, 0] == (16 * (v[3] + v[4]) + 16) // 32 == 45  # the right tap is unused: T = 32
    assert out[0, 6, 0] == (16 * (v[6] + v[7]) + 16) // 32 == 75  # the left tap is unused
    assert out[0, 3, 0] == 40                                      # both used
    wide = prefilter_ref(row_img(), d, 8, 1.0, 8, 3.0)             # |3| <= 3: used again
    assert wide[0, 4, 0] == 50


def test_nan_and_inf_in_the_map():
    d = np.full((1, 9), delta_for_half_width(16), f32)
    d[0, 2], d[0, 4], d[0, 6] = np.nan, np.inf, -np.inf
    img = row_img()
    out = prefilter_ref(img, d, 8, 1.0, 8, 1.0)
    for x in (2, 4, 6):
        assert np.array_equal(out[0, x], img[0, x])  # H = 0
    v = ROW[0].astype(int)
    assert out[0, 1, 0] == (16 * (v[0] + v[1]) + 16) // 32  # the NaN tap at 2 is unused
    assert out[0, 3, 0] == 16 * v[3] // 16                  # NaN on one side, inf on the other: both unused
    assert out[0, 7, 0] == (16 * (v[7] + v[8]) + 16) // 32
    assert half_width(f32(1e38), 8, 8.0, 16, gain=8.0) == 0  # gain * delta overflows: not finite


def test_screen_plane_is_byte_identical():
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (3, 40, 3)).astype(np.uint8)
    gain, conv = 0.75, 9.0
    d = np.full((3, 40), f32(conv) / f32(gain), f32)
    assert np.array_equal(prefilter_ref(img, d, 8, 4.0, 16, 100.0, gain, conv), img)


def test_vectorised_form_equals_the_scalar_statement():
    rng = np.random.RandomState(11)
    for (rows, cols, N, strength, radius, gate, gain, conv) in ((3, 1, 8, 1.0, 16, 1.0, 1.0, 0.0), (2, 3, 8, 2.0, 16, 50.0, 1.0, 0.0),
                                                                (4, 37, 8, 1.0, 8, 1.0, 1.0, 0.0), (3, 70, 5, 1.7, 3, 0.5, 0.6, -4.0),
                                                                (2, 50, 2, 0.3, 16, 2.0, 2.0, 11.0), (2, 33, 8, 0.0, 4, 1.0, 1.0, 0.0)):
        img = rng.randint(0, 256, (rows, cols, 4)).astype(np.uint8)
        d = (rng.randint(-160, 161, (rows, cols)) / 4.0).astype(f32)
        d[:, cols // 2:] = np.round(d[:, cols // 2:] / 8) * 8  # runs of equal depth, so taps are used
        if cols > 8:
            d[0, 3], d[0, 5], d[rows - 1, cols - 2] = np.nan, np.inf, -np.inf
        a = prefilter_ref(img, d, N, strength, radius, gate, gain, conv)
        b = prefilter_vec(img, d, N, strength, radius, gate, gain, conv)
        assert np.array_equal(a, b), (rows, cols, N)


def test_no_background_output_depends_on_the_foreground():
    """a sharp in-plane foreground beside a background at delta = 28, gate 1: the blurred background never pulls in a foreground colour"""
    rng = np.random.RandomState(5)
    cols, edge = 64, 30
    img = rng.randint(0, 256, (2, cols, 3)).astype(np.uint8)
    d = np.zeros((2, cols), f32)
    d[:, edge:] = 28.0
    a = prefilter_ref(img, d, 8, 1.0, 8, 1.0)
    other = img.copy()
    other[:, :edge] = 255 - other[:, :edge]
    b = prefilter_ref(other, d, 8, 1.0, 8, 1.0)
    assert np.array_equal(a[:, edge:], b[:, edge:])
    assert np.array_equal(a[:, :edge], img[:, :edge])      # the foreground is on the screen plane: untouched
    assert not np.array_equal(a[:, edge:], img[:, edge:])  # the background is blurred
    # with the gate open the leak is there: this is what the gate is for
    c = prefilter_ref(other, d, 8, 1.0, 8, 100.0)
    assert not np.array_equal(prefilter_ref(img, d, 8, 1.0, 8, 100.0)[:, edge:], c[:, edge:])


# ----------------------------------------------------------------------------- quality, on the oracle's renderer
def aperture_errors(orc, delta, N=8, v=3, rows=64, cols=256, border=64):
    """mean abs error of view v against the float mean of the oracle's dibr_dbm at 16 positions across the view's aperture
    s_v +- 1 / (2 (N - 1)), from the unfiltered and from the prefiltered pair (strength 1, max_radius 8, gate 1)"""
    rng = np.random.RandomState(7)
    L = rng.randint(0, 256, (rows, cols, 3)).astype(np.uint8)
    R = np.roll(L, delta, axis=1)  # fronto-parallel: x_right = x_left + delta
    d = np.full((rows, cols), delta, f32)
    one = np.ones((rows, cols), f32)
    s_v = float(f32(1.0 - float(f32(v)) / (float(f32(N)) - 1.0)))
    ideal = np.zeros((rows, cols, 3), np.float64)
    for i in range(16):
        s = s_v + ((i + 0.5) / 16.0 - 0.5) / (N - 1)
        ideal += orc.dibr_dbm(L, R, d, d, one, one, s)
    ideal /= 16.0
    Lf, Rf = prefilter_ref(L, d, N, 1.0, 8, 1.0), prefilter_ref(R, d, N, 1.0, 8, 1.0)
    inner = slice(border, cols - border)
    plain = np.abs(orc.dibr_dbm(L, R, d, d, one, one, s_v)[:, inner] - ideal[:, inner]).mean()
    filtered = np.abs(orc.dibr_dbm(Lf, Rf, d, d, one, one, s_v)[:, inner] - ideal[:, inner]).mean()
    return plain, filtered


@pytest.mark.parametrize("delta", [28, 7])
def test_prefiltered_view_is_closer_to_the_aperture_mean(orc, delta):
    plain, filtered = aperture_errors(orc, delta)
    print("delta %d: mean abs error %.2f unfiltered, %.2f prefiltered" % (delta, plain, filtered))
    assert filtered < plain


# ----------------------------------------------------------------------------- the tools
@pytest.mark.parametrize("tool, nargs", [("stm_video", 16), ("stm_image", 17)])
def test_tools_refuse_a_malformed_antialias_option(capsys, tool, nargs):
    """--antialias needs three numbers inside the library's ranges (usage and -1, nothing run)"""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location(tool, os.path.join(ROOT, "tools", tool + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for tail in (["--antialias", "1.0", "8"], ["--antialias", "1.0", "x", "1.0"], ["--antialias", "9.0", "8", "1.0"],
                 ["--antialias", "1.0", "0", "1.0"], ["--antialias", "1.0", "17", "1.0"], ["--antialias", "1.0", "8", "-1.0"],
                 ["--antialias", "nan", "8", "1.0"], ["--antialias", "1.0", "8", "inf"], ["--antialias", "1.0", "8.5", "1.0"]):
        assert mod.main([tool] + ["x"] * (nargs - 1) + tail) == -1, tail
        assert "--antialias STRENGTH MAX_RADIUS GATE" in capsys.readouterr().out
