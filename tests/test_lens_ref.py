"""Calibrated lenticular interlacing (stm_set_lens, stm_mux_multiview_lens): the numpy statement of the definition in
include/stm_hip.h that the GPU tests (test_gpu_lens.py) compare against bit for bit -- tied to the oracle's interlacer at the one
geometry the reference's formula describes -- its known answers, the frame composed from the oracle's stages, and that rendering
every sub-pixel at its own continuous position brings a slanted analytic scene closer to what that sub-pixel should show.  No GPU."""
import numpy as np
import pytest

from test_interp_ref import interp_frame
from test_linwarp_ref import INTERP, HSLO, LINEAR_WARP, SUBPIXEL, _true_view, dbm_ref, linwarp_frame
from test_subpixel_ref import _P, _slanted_pair

f32 = np.float32


# ----------------------------------------------------------------------------- the definition
def lens_phase_ref(Ho, Wo, pitch, slope, centre):
    """a[ty][tx][c]: the lens phase of byte c (sub-pixel k = 2 - c) of output pixel (tx, ty); float64, one operation per line"""
    ty = np.arange(Ho, dtype=np.float64)[:, None, None]
    s = (3 * np.arange(Wo, dtype=np.int64)[None, :, None] + (2 - np.arange(3, dtype=np.int64))[None, None, :]).astype(np.float64)
    with np.errstate(all="ignore"):
        t1 = ty * np.float64(slope)
        t2 = s + t1
        t3 = t2 / np.float64(pitch)
        t4 = t3 + np.float64(centre)
        a = t4 - np.floor(t4)
        return np.where(a < 1.0, a, 0.0)  # a >= 1.0 (and a t4 that is not finite) -> 0


def lens_pick_ref(a, N, mode):
    """mode 1: (v, None, None); mode 2: (v0, w, None); mode 3: (None, None, shift)"""
    g = a * np.float64(N)
    if mode == 1:
        return np.minimum(g.astype(np.int64), N - 1), None, None
    g = g - 0.5
    g = np.minimum(np.maximum(g, 0.0), np.float64(N - 1))
    if mode == 2:
        v0 = np.minimum(g.astype(np.int64), N - 2)
        return v0, (g - v0.astype(np.float64)).astype(f32), None
    u = g / np.float64(N - 1)
    return None, None, (1.0 - u).astype(f32)


def sample_grid(Ho, Wo, Hin, Win):
    """The reference's sampling position of every output pixel and the 4-neighbour sampler's taps (d_mux_multiview.cu:10-36, :44-49):
    (x0, x1, wx) per column, (y0, y1, wy) per row, float32 one operation per line"""
    def axis(n_out, n_in):
        t = (np.arange(n_out, dtype=f32) / f32(n_out)).astype(f32)
        t = (t * f32(n_in)).astype(f32)
        t = np.fmin(np.fmax(t, f32(0)), f32(n_in - 1))
        i0 = np.floor(t).astype(np.int64)
        return i0, np.minimum(i0 + 1, n_in - 1), (t - i0.astype(f32)).astype(f32)
    return axis(Wo, Win), axis(Ho, Hin)


def combine4(v00, v01, v10, v11, wx, wy):
    """fast_bilinear_interp's arithmetic on the four neighbours' u8 values ([Ho][Wo] each; wx [1][Wo], wy [Ho][1]); u8 truncation"""
    a = (v00.astype(f32) * (f32(1) - wx)).astype(f32)
    b = (v01.astype(f32) * wx).astype(f32)
    top = (a + b).astype(f32)
    a = (v10.astype(f32) * (f32(1) - wx)).astype(f32)
    b = (v11.astype(f32) * wx).astype(f32)
    bot = (a + b).astype(f32)
    a = (top * (f32(1) - wy)).astype(f32)
    b = (bot * wy).astype(f32)
    return (a + b).astype(f32).astype(np.uint8)


def blend2(A, B, w):
    p = (A.astype(f32) * (f32(1) - w)).astype(f32)
    q = (B.astype(f32) * w).astype(f32)
    return (p + q).astype(f32).astype(np.uint8)


def mux_lens_ref(views, mode, pitch, slope, centre, Ho, Wo):
    """stm_mux_multiview_lens, modes 1 and 2: [Ho][Wo][3] from the list of N views ([H][W][E], bytes 0..2 read)"""
    assert mode in (1, 2)
    N = len(views)
    Hin, Win, _ = views[0].shape
    (x0, x1, wx), (y0, y1, wy) = sample_grid(Ho, Wo, Hin, Win)
    wx, wy = wx[None, :], wy[:, None]
    a = lens_phase_ref(Ho, Wo, pitch, slope, centre)
    v, w, _ = lens_pick_ref(a, N, mode)
    stack = np.stack([np.asarray(x)[..., :3] for x in views])  # [N][H][W][3]
    # every view resampled at every output pixel: [N][Ho][Wo][3]
    res = np.stack([np.stack([combine4(stack[n][y0[:, None], x0[None, :], c], stack[n][y0[:, None], x1[None, :], c],
                                       stack[n][y1[:, None], x0[None, :], c], stack[n][y1[:, None], x1[None, :], c], wx, wy)
                              for c in range(3)], axis=-1) for n in range(N)])
    yy, xx, cc = np.meshgrid(np.arange(Ho), np.arange(Wo), np.arange(3), indexing="ij")
    A = res[v, yy, xx, cc]
    if mode == 1:
        return A
    return blend2(A, res[v + 1, yy, xx, cc], w)


def render_chain(orc, L, R, dl, dr):
    """what the renderer derives from the two images and maps once per frame: the masks and the blend G(1 - mask_r)"""
    occl_l, occl_r = orc.dibr_occl(dl, dr)
    occl_l, occl_r = orc.filter_bleed_1(occl_l, 1), orc.filter_bleed_1(occl_r, 1)
    ml, mr = orc.dibr_occl_to_mask(occl_l, occl_r)
    tm = orc.filter_gaussian_1((f32(1) - mr).astype(f32), 10, 15.0)
    return dict(L=L, R=R, dl=dl, dr=dr, ml=ml, mr=mr, tm=tm)


def _tap(img, Y, X, fx, c, linear):
    """warp_tap: channel c of row Y at the clamped position fx ([Ho][Wo] each)"""
    W = img.shape[1]
    if not linear:
        return img[Y, fx.astype(np.int64), c]
    i0 = np.floor(fx).astype(np.int64)
    i1 = np.minimum(i0 + 1, W - 1)
    wx = (fx - i0.astype(f32)).astype(f32)
    a = (img[Y, i0, c].astype(f32) * (f32(1) - wx)).astype(f32)
    b = (img[Y, i1, c].astype(f32) * wx).astype(f32)
    return (a + b).astype(f32).astype(np.uint8)


def sample_shift_ref(ch, Y, X, shift, c, linear):
    """The renderer's general form at neighbour (X, Y) and the per-sub-pixel `shift` ([Ho][Wo] each), channel c: both backward warps,
    masks, blend, u8 wrap -- float32, one operation per line"""
    W = ch["L"].shape[1]
    with np.errstate(all="ignore"):
        shift_l = (-shift).astype(f32)
        shift_r = (1.0 - shift.astype(np.float64)).astype(f32)
        sd = (ch["dr"][Y, X] * shift_l).astype(f32)
        fx = (X.astype(f32) + sd).astype(f32)
        fxl = np.fmin(np.fmax(fx, f32(0)), f32(W - 1))
        sd = (ch["dl"][Y, X] * shift_r).astype(f32)
        fx = (X.astype(f32) + sd).astype(f32)
        fxr = np.fmin(np.fmax(fx, f32(0)), f32(W - 1))
        m = ch["tm"][Y, X]
        pa = (_tap(ch["L"], Y, X, fxl, c, linear).astype(f32) * ch["mr"][Y, X]).astype(f32).astype(np.uint8)
        pb = (_tap(ch["R"], Y, X, fxr, c, linear).astype(f32) * ch["ml"][Y, X]).astype(f32).astype(np.uint8)
        cb = ((f32(1) - m) * pa.astype(f32)).astype(f32)
        ca = (m * pb.astype(f32)).astype(f32)
        return (cb.astype(np.uint8) + ca.astype(np.uint8)).astype(np.uint8)


def chain_views(orc, ch, N, linear):
    """the N views of the frame: [right image, N - 2 synthesised ones (dbm_ref at the view's shift), left image]"""
    views = [ch["R"]]
    for v in range(1, N - 1):
        shift = float(f32(1.0 - (1.0 * float(f32(v))) / (float(f32(N)) - 1.0)))
        views.append(dbm_ref(orc, ch["L"], ch["R"], ch["dl"], ch["dr"], ch["ml"], ch["mr"], shift, linear, tm=ch["tm"]))
    views.append(ch["L"])
    return views


def render_lens_ref(orc, ch, N, lens, linear, Ho, Wo):
    """The frame's render under the lens geometry lens = (mode, pitch, slope, centre) from a render_chain: modes 1 and 2 interlace
    the frame's views, mode 3 renders every sub-pixel at its own shift.  Returns [Ho][Wo][3]."""
    mode, pitch, slope, centre = lens
    if mode in (1, 2):
        return mux_lens_ref(chain_views(orc, ch, N, linear), mode, pitch, slope, centre, Ho, Wo)
    assert mode == 3
    H, W, _ = ch["L"].shape
    (x0, x1, wx), (y0, y1, wy) = sample_grid(Ho, Wo, H, W)
    _, _, shift = lens_pick_ref(lens_phase_ref(Ho, Wo, pitch, slope, centre), N, 3)
    X0, X1 = np.broadcast_to(x0[None, :], (Ho, Wo)), np.broadcast_to(x1[None, :], (Ho, Wo))
    Y0, Y1 = np.broadcast_to(y0[:, None], (Ho, Wo)), np.broadcast_to(y1[:, None], (Ho, Wo))
    out = np.zeros((Ho, Wo, 3), np.uint8)
    for c in range(3):
        s = shift[..., c]
        out[..., c] = combine4(sample_shift_ref(ch, Y0, X0, s, c, linear), sample_shift_ref(ch, Y0, X1, s, c, linear),
                               sample_shift_ref(ch, Y1, X0, s, c, linear), sample_shift_ref(ch, Y1, X1, s, c, linear),
                               wx[None, :], wy[:, None])
    return out


_CHAINS = {}


def frame_chain(orc, sbs, p, extra_bits=0):
    """The oracle chain of a frame up to what the renderer needs (test_interp_ref.interp_frame's maps of stages 2 with the 0x100 /
    0x200 / 0x400 bits of extra_bits, then render_chain); computed once per (frame, parameters, bits), read only"""
    key = (sbs.tobytes(), sbs.shape, tuple(sorted(vars(p).items())), extra_bits & (HSLO | SUBPIXEL | INTERP))
    if key not in _CHAINS:
        W = sbs.shape[1] // 2
        dl, dr, _, info = interp_frame(orc, sbs, p, 2, bool(extra_bits & INTERP), subpixel=bool(extra_bits & SUBPIXEL),
                                       hslo=bool(extra_bits & HSLO))
        ch = render_chain(orc, info["img_l"], info["img_r"], dl, dr)
        for a in ch.values():
            a.setflags(write=False)
        _CHAINS[key] = ch
    return _CHAINS[key]


def frame_lens_ref(orc, sbs, p, lens, extra_bits=0, out_rows=None, out_cols=None):
    """The frame under a lens geometry, composed from the oracle's stages: (disp_l, disp_r, interlaced).  extra_bits: the frame's
    `stages` bits 0x100 / 0x200 / 0x400 (the maps) and 0x800 (linear warps)."""
    H, W = sbs.shape[0], sbs.shape[1] // 2
    ch = frame_chain(orc, sbs, p, extra_bits)
    out = render_lens_ref(orc, ch, p.num_views, lens, bool(extra_bits & LINEAR_WARP), out_rows or H, out_cols or W)
    return ch["dl"], ch["dr"], out


# ----------------------------------------------------------------------------- shared inputs
def random_views(seed, N, H, W, elem_sz=3):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=(H, W, elem_sz)).astype(np.uint8) for _ in range(N)]


def flat_views(N, H=4, W=6, step=10):
    """view n holds n * step in every byte: an interlaced byte names the view it came from"""
    return [np.full((H, W, 3), n * step, np.uint8) for n in range(N)]


# ----------------------------------------------------------------------------- tie to the reference
@pytest.mark.parametrize("sizes", [((32, 64), (32, 64)), ((37, 53), (50, 81))], ids=["32x64", "37x53_to_50x81"])
def test_pitch_n_slope_1_is_the_references_interlacer(orc, sizes):
    """N = 8 views, angle 18.43: y_interval = 8.0023 and the reference's row offset int((ty % 8 + 1) * 8 / y_interval) is ty % 8, so its
    view of sub-pixel k is (3 tx + k + ty) mod 8 -- pitch 8, slope 1; centre 1/16 puts every phase on a bin centre"""
    (H, W), (Ho, Wo) = sizes
    N, angle = 8, 18.43
    a = f32(f32(angle) * f32(3.1415926535))
    yi = f32(float(f32(N)) / np.tan(float(a) / 180.0) / float(f32(3)))
    assert abs(float(yi) - 8.002303) < 1e-5
    ymod = int(np.round(yi))
    inv_y = f32(1) / yi
    ty = np.arange(Ho)
    off = ((((ty % ymod).astype(f32) + f32(1)) * f32(N)).astype(f32) * inv_y).astype(f32).astype(np.int64)
    assert ymod == 8 and np.array_equal(off, ty % 8)
    views = random_views(7 + H, N, H, W)
    got = mux_lens_ref(views, 1, 8.0, 1.0, 1.0 / 16.0, Ho, Wo)
    assert np.array_equal(got, orc.mux_multiview(views, angle, Ho, Wo))


# ----------------------------------------------------------------------------- known answers
def test_tiny_negative_t4_takes_the_guard():
    """row 1, sub-pixel s = 0 with slope -1e-30: t4 = -1.25e-31, floor = -1, t4 + 1 rounds to 1.0 -> a = 0 (view 0), not a * N = N"""
    a = lens_phase_ref(2, 2, 8.0, -1e-30, 0.0)
    assert a[1, 0, 2] == 0.0 and a[0, 0, 2] == 0.0
    t4 = (0.0 + 1.0 * -1e-30) / 8.0
    assert t4 < 0 and t4 - np.floor(t4) == 1.0  # what the guard catches
    assert a[1, 0, 1] == 0.125 and a[1, 1, 2] == 0.375
    out = mux_lens_ref(flat_views(8, 2, 2), 1, 8.0, -1e-30, 0.0, 2, 2)
    assert out[1, 0].tolist() == [20, 10, 0] and out[1, 1].tolist() == [50, 40, 30]
    assert mux_lens_ref(flat_views(8, 2, 2), 2, 8.0, -1e-30, 0.0, 2, 2)[1, 0, 2] == 0


@pytest.mark.parametrize("mode", [1, 2])
def test_whole_number_centres_change_nothing(mode):
    views = random_views(3, 5, 9, 14)
    for pitch, slope in ((8.0, 1.0), (4.0, -0.5)):  # dyadic: t3 + centre is exact
        want = mux_lens_ref(views, mode, pitch, slope, 0.25, 9, 14)
        for k in (1.0, -2.0, 5.0):
            assert np.array_equal(mux_lens_ref(views, mode, pitch, slope, 0.25 + k, 9, 14), want)
    assert not np.array_equal(mux_lens_ref(views, mode, 8.0, 1.0, 0.5, 9, 14), mux_lens_ref(views, mode, 8.0, 1.0, 0.25, 9, 14))


def test_negative_slope_and_byte_order():
    """pitch 8, slope -1, centre 1/16: byte c of (tx, ty) shows view (3 tx + (2 - c) - ty) mod 8; R (byte 2) is the first sub-pixel"""
    N, H, W = 8, 11, 7
    out = mux_lens_ref(flat_views(N, H, W), 1, 8.0, -1.0, 1.0 / 16.0, H, W)
    ty, tx, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    assert np.array_equal(out, (((3 * tx + (2 - c) - ty) % 8) * 10).astype(np.uint8))


def test_non_integer_pitch_walks_through_the_views():
    """pitch 7.5 with 5 views: sub-pixel s of row 0 shows view int(frac(s / 7.5) * 5)"""
    out = mux_lens_ref(flat_views(5, 1, 10), 1, 7.5, 0.0, 0.0, 1, 10)
    s = 3 * np.arange(10)[:, None] + (2 - np.arange(3))[None, :]
    assert np.array_equal(out[0], (np.floor((s / 7.5 - np.floor(s / 7.5)) * 5).astype(np.int64) * 10).astype(np.uint8))


def test_mode_2_at_weight_0_is_mode_1():
    """centre 1/16 with pitch = N = 8: g = a N - 0.5 is a whole number m, so w = 0 (or w = 1 on view 6 -> 7 for m = 7) and the blend
    is view m alone: mode 1's"""
    views = random_views(5, 8, 12, 20)
    for Ho, Wo in ((12, 20), (17, 31)):
        assert np.array_equal(mux_lens_ref(views, 2, 8.0, 1.0, 1.0 / 16.0, Ho, Wo), mux_lens_ref(views, 1, 8.0, 1.0, 1.0 / 16.0, Ho, Wo))
    assert not np.array_equal(mux_lens_ref(views, 2, 8.0, 1.0, 0.0, 12, 20), mux_lens_ref(views, 1, 8.0, 1.0, 0.0, 12, 20))


def test_mode_2_blends_neighbours_and_never_the_end_views():
    """5 views, pitch 5, slope 0: a N = s mod 5, g = s mod 5 - 0.5 -> the end half-bin (s mod 5 = 0) shows view 0 unblended, the rest
    the mean of views m - 1 and m, truncated"""
    out = mux_lens_ref(flat_views(5, 1, 5, step=11), 2, 5.0, 0.0, 0.0, 1, 5)
    s = 3 * np.arange(5)[:, None] + (2 - np.arange(3))[None, :]
    m = s % 5
    want = np.where(m == 0, 0, np.floor(((m - 1) * 11) * 0.5 + (m * 11) * 0.5)).astype(np.uint8)
    assert np.array_equal(out[0], want)
    top = mux_lens_ref(flat_views(5, 1, 5, step=11), 2, 5.0, 0.0, 0.95, 1, 5)  # a N = m + 4.75 mod 5: the last half-bin and beyond
    assert set(np.unique(top)) <= {44, 0, 2, 13, 24, 35}  # view 4 alone, view 0 alone, or neighbours at w = 0.25: never 4 with 0


def test_two_views():
    """N = 2, pitch 2, slope 0: even sub-pixels a = 0 -> view 0; odd ones a = 0.5 -> mode 1 view 1, mode 2 g = 0.5: (10 + 21) / 2 -> 15"""
    views = [np.full((1, 4, 3), 10, np.uint8), np.full((1, 4, 3), 21, np.uint8)]
    s = 3 * np.arange(4)[:, None] + (2 - np.arange(3))[None, :]
    assert np.array_equal(mux_lens_ref(views, 1, 2.0, 0.0, 0.0, 1, 4)[0], np.where(s % 2 == 0, 10, 21))
    assert np.array_equal(mux_lens_ref(views, 2, 2.0, 0.0, 0.0, 1, 4)[0], np.where(s % 2 == 0, 10, 15))


# ----------------------------------------------------------------------------- composition
def _small_frame():
    from stm_amd import synth
    H, W, D, zd = 40, 64, 16, 8
    return synth.sbs_frame(H, W, D, zd)[0], _P(D, zd, usd=17, lsd=8), H, W


@pytest.mark.parametrize("extra", [0, SUBPIXEL | LINEAR_WARP], ids=["plain", "subpixel_linear"])
def test_frame_modes_1_and_2_interlace_the_frames_views(orc, extra):
    """frame_lens_ref in modes 1 and 2 is mux_lens_ref on the views test_linwarp_ref.linwarp_frame composes; the maps are the frame's"""
    sbs, p, H, W = _small_frame()
    dl, dr, _, views = linwarp_frame(orc, sbs, p, extra & SUBPIXEL, linear=bool(extra & LINEAR_WARP))
    for mode in (1, 2):
        for Ho, Wo in ((H, W), (50, 81)):
            lens = (mode, 7.37, 0.86, 0.3)
            gl, gr, out = frame_lens_ref(orc, sbs, p, lens, extra, Ho, Wo)
            assert np.array_equal(gl, dl) and np.array_equal(gr, dr)
            assert np.array_equal(out, mux_lens_ref(views, *lens, Ho, Wo)), (mode, Ho)


@pytest.mark.parametrize("extra", [0, SUBPIXEL | LINEAR_WARP], ids=["plain", "subpixel_linear"])
def test_mode_3_on_a_bin_centre_is_the_discrete_view(orc, extra):
    """pitch = N = 8, slope 1, centre 1/16: every phase sits on the centre of bin m = (s + ty) mod 8, where mode 3's shift is view m's
    own -- for the interior views 1 .. 6 the sample is the view's; views 0 and 7 are the two images there, a warp here"""
    sbs, p, H, W = _small_frame()
    for Ho, Wo in ((H, W), (50, 81)):
        near = frame_lens_ref(orc, sbs, p, (1, 8.0, 1.0, 1.0 / 16.0), extra, Ho, Wo)[2]
        cont = frame_lens_ref(orc, sbs, p, (3, 8.0, 1.0, 1.0 / 16.0), extra, Ho, Wo)[2]
        ty, tx, c = np.meshgrid(np.arange(Ho), np.arange(Wo), np.arange(3), indexing="ij")
        m = (3 * tx + (2 - c) + ty) % 8
        inner = (m >= 1) & (m <= 6)
        assert np.array_equal(near[inner], cont[inner])
        assert not np.array_equal(near[~inner], cont[~inner])
    off_centre = frame_lens_ref(orc, sbs, p, (3, 8.0, 1.0, 0.0), extra)[2]
    assert not np.array_equal(off_centre, frame_lens_ref(orc, sbs, p, (1, 8.0, 1.0, 0.0), extra)[2])


# ----------------------------------------------------------------------------- quality
PANEL = (7.37, 0.86, 0.3)


def _lens_errors(orc, H, W, a, b, D, zd, subpixel, N=8, m=16):
    """mean |sub-pixel - the true scene seen from that sub-pixel's own position| over the interior, modes 1 / 2 / 3, linear warps"""
    L, R, _ = _slanted_pair(H, W, a, b)
    sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
    p = _P(D, zd)
    extra = LINEAR_WARP | (SUBPIXEL if subpixel else 0)
    _, _, shift = lens_pick_ref(lens_phase_ref(H, W, *PANEL), N, 3)  # the position the sub-pixel's lens phase points at
    truth = np.stack([_true_view(H, W, a, b, shift[..., c].astype(np.float64))[..., c] for c in range(3)], axis=-1)
    errs = []
    for mode in (1, 2, 3):
        out = frame_lens_ref(orc, sbs, p, (mode,) + PANEL, extra)[2]
        errs.append(float(np.mean(np.abs(out[m:-m, m:-m].astype(np.float64) - truth[m:-m, m:-m]))))
    return errs


@pytest.mark.parametrize("subpixel", [False, True], ids=["whole_pixel_maps", "subpixel_maps"])
def test_continuous_views_bring_the_sub_pixels_closer_to_the_truth(orc, subpixel):
    """96 x 200 slanted pair, t(x) = -11 + 0.11 x, D = 32, zd = 16, linear warps, panel pitch 7.37 / slope 0.86 / centre 0.3, 8 views,
    16-pixel margin; mean error of modes 1 / 2 / 3:
      maps of stages 2:         1.088 / 0.919 / 0.796   (mode 3 / mode 1 = 0.73)
      maps of stages 2 | 0x200: 1.080 / 0.913 / 0.782   (0.72)
    The gain is the removed quantisation of the view position (a sub-pixel up to half a bin from its view's camera sees the scene
    displaced by up to |t| / 14), so it scales with the disparity.  The bound 0.85 leaves room for nothing but a bug."""
    e1, e2, e3 = _lens_errors(orc, 96, 200, -11.0, 0.11, 32, 16, subpixel)
    print("large-disparity pair, sub-pixel %d: mode 1 %.3f, mode 2 %.3f, mode 3 %.3f (ratio %.2f)" % (subpixel, e1, e2, e3, e3 / e1))
    assert e3 < 0.85 * e1, (e1, e2, e3)


@pytest.mark.parametrize("subpixel", [False, True], ids=["whole_pixel_maps", "subpixel_maps"])
def test_small_disparity_pair_figures(orc, subpixel):
    """The pair of test_linwarp_ref (96 x 160, t(x) = -2.3 + 0.03 x, |t| <= 2.5, D = 16, zd = 8) on the same panel, printed only: with
    so little disparity the view-position quantisation is worth a few hundredths of a grey level and the modes differ by no more:
      maps of stages 2:         0.615 / 0.707 / 0.679
      maps of stages 2 | 0x200: 0.537 / 0.673 / 0.551
    (modes 2 and 3 lose the end views' shortcut to the unwarped images near the lens edges, which costs about what the continuous
    position gains here)."""
    e1, e2, e3 = _lens_errors(orc, 96, 160, -2.3, 0.03, 16, 8, subpixel)
    print("small-disparity pair, sub-pixel %d: mode 1 %.3f, mode 2 %.3f, mode 3 %.3f" % (subpixel, e1, e2, e3))
    assert all(np.isfinite(e) for e in (e1, e2, e3))


# ----------------------------------------------------------------------------- the tools' option
def test_tools_refuse_a_malformed_lens_option(capsys):
    """--lens needs its four values; stm_image.py interlaces finished views, so it takes modes 1 and 2 only (usage and -1, nothing run)"""
    import importlib.util
    import os
    from conftest import ROOT
    for tool, tail in (("stm_video", ["--lens", "3", "7.37", "0.86"]), ("stm_image", ["--lens", "3", "7.37", "0.86", "0.3"]),
                       ("stm_image", ["--lens", "1", "7.37"])):
        spec = importlib.util.spec_from_file_location(tool, os.path.join(ROOT, "tools", tool + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert mod.main([tool] + ["x"] * 16 + tail) == -1
        assert "--lens MODE PITCH SLOPE CENTRE" in capsys.readouterr().out
