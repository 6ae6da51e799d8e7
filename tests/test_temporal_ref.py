"""Temporal disparity stabilisation (stm_disp_temporal, the frame bit 0x2000 of stm_d_adcensus_stm_t and of the frame stream): the
numpy float32 statement of the definition in include/stm_hip.h that the GPU tests (test_gpu_temporal.py) compare against bit
for bit -- a vectorised form tied element by element to a plain scalar loop --, its known answers, and what it does to the maps
of the oracle chain on a static noisy scene and around a moving object.  No GPU."""
import numpy as np
import pytest

from test_interp_ref import interp_frame
from test_linwarp_ref import dbm_ref
from test_subpixel_ref import _P

HSLO, SUBPIXEL, INTERP, LINEAR_WARP, TEMPORAL = 0x100, 0x200, 0x400, 0x800, 0x2000
ALPHA, THRESH_COLOR, THRESH_DISP = 0.5, 24, 1.5  # the frame's defaults (stm_hip.h)


def sad_map(img, img_prev):
    """sad(q): int32 [H][W], the summed absolute difference of the first three bytes of every pixel"""
    a, b = img[..., :3].astype(np.int32), img_prev[..., :3].astype(np.int32)
    return np.abs(a - b).sum(axis=-1).astype(np.int32)


def sad_max(img, img_prev):
    """m(p): the maximum of sad over the 3 x 3 pixels around p that lie inside the image.  sad >= 0 and every neighbourhood holds
    its own centre, so a border of zeros takes no part in any maximum: that is the clipped neighbourhood (temporal_loop walks it
    pixel by pixel)."""
    sad = sad_map(img, img_prev)
    H, W = sad.shape
    pad = np.zeros((H + 2, W + 2), np.int32)
    pad[1:-1, 1:-1] = sad
    m = sad.copy()
    for j in range(3):
        for i in range(3):
            m = np.maximum(m, pad[j:j + H, i:i + W])
    return m


def temporal_ref(cur, prev, img, img_prev, alpha=ALPHA, thresh_color=THRESH_COLOR, thresh_disp=THRESH_DISP):
    """The definition on whole arrays, one float32 operation per line.  Returns the new map; nothing passed in is modified."""
    f = np.float32
    c = np.ascontiguousarray(cur, dtype=f)
    q = np.ascontiguousarray(prev, dtype=f)
    m = sad_max(img, img_prev)
    with np.errstate(all="ignore"):
        t = (q - c).astype(f)
        df = np.abs(t)
        u = (f(alpha) * t).astype(f)
        o = (c + u).astype(f)
        gate = (m <= int(thresh_color)) & (df <= f(thresh_disp))  # a NaN in df compares false
    out = np.where(gate, o, c)
    assert out.dtype == f
    return out


def temporal_loop(cur, prev, img, img_prev, alpha=ALPHA, thresh_color=THRESH_COLOR, thresh_disp=THRESH_DISP):
    """The definition read aloud, one pixel at a time"""
    f = np.float32
    H, W = cur.shape
    out = np.array(cur, dtype=f)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                m = 0
                for j in (-1, 0, 1):
                    for i in (-1, 0, 1):
                        qy, qx = y + j, x + i
                        if 0 <= qy < H and 0 <= qx < W:
                            s = sum(abs(int(img[qy, qx, k]) - int(img_prev[qy, qx, k])) for k in range(3))
                            m = max(m, s)
                c, q = f(cur[y, x]), f(prev[y, x])
                t = f(q - c)
                df = f(abs(t))
                if m <= thresh_color and df <= f(thresh_disp):
                    u = f(f(alpha) * t)
                    out[y, x] = f(c + u)
    return out


def render_ref(orc, L, R, dl, dr, p, linear=False, out_rows=None, out_cols=None):
    """The frame's renderer on given maps, composed from the oracle's stages as test_linwarp_ref.linwarp_frame composes it: hit
    maps, bleed, masks, dbm_ref per view, the oracle's interlacer.  Returns the interlaced frame."""
    H, W = dl.shape
    occl_l, occl_r = orc.dibr_occl(dl, dr)
    occl_l, occl_r = orc.filter_bleed_1(occl_l, 1), orc.filter_bleed_1(occl_r, 1)
    ml, mr = orc.dibr_occl_to_mask(occl_l, occl_r)
    tm = orc.filter_gaussian_1((np.float32(1) - mr).astype(np.float32), 10, 15.0)
    N = p.num_views
    views = [R]
    for v in range(1, N - 1):
        shift = float(np.float32(1.0 - (1.0 * float(np.float32(v))) / (float(np.float32(N)) - 1.0)))
        views.append(dbm_ref(orc, L, R, dl, dr, ml, mr, shift, linear, tm=tm))
    views.append(L)
    return orc.mux_multiview(views, p.angle, out_rows or H, out_cols or W)


def halves(sbs):
    """the left and the right view of a side-by-side frame [H][2W][E]"""
    W = sbs.shape[1] // 2
    return np.ascontiguousarray(sbs[:, :W]), np.ascontiguousarray(sbs[:, W:2 * W])


def temporal_recursion(frames, maps, alpha=ALPHA, thresh_color=THRESH_COLOR, thresh_disp=THRESH_DISP):
    """What a frame sequence computes: frames[k] the side-by-side inputs, maps[k] = (disp_l, disp_r) of frame k without the step.
    Frame 0 passes through; frame k is temporal_ref of its own maps against frame k - 1's OUTPUT, each view on its own half."""
    out = []
    for k, (sbs, (dl, dr)) in enumerate(zip(frames, maps)):
        if k == 0:
            out.append((dl.copy(), dr.copy()))
            continue
        (L, R), (Lp, Rp) = halves(sbs), halves(frames[k - 1])
        out.append((temporal_ref(dl, out[-1][0], L, Lp, alpha, thresh_color, thresh_disp),
                    temporal_ref(dr, out[-1][1], R, Rp, alpha, thresh_color, thresh_disp)))
    return out


# ----------------------------------------------------------------------------- shared inputs
# 1 x 1, 3 x 5, 40 x 72, 67 x 131 (ragged against any tile), widths 63 / 64 / 65 around the 64-wide tile, 150 rows = several blocks tall
SHAPES = [(1, 1), (3, 5), (40, 72), (67, 131), (5, 63), (5, 64), (18, 65), (150, 9)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]


def temporal_case(seed, H, W, elem_sz=3, nonfinite=True):
    """Random inputs of one call: an image pair that differs by a little noise nearly everywhere (sad around the default gate,
    on both sides of it) and by a lot in a few patches, maps that differ by less and by more than the default thresh_disp, and
    -- nonfinite -- NaN and +-inf in either map.  Bytes past a pixel's third are random in both images (never read)."""
    rng = np.random.RandomState(seed)
    img_prev = rng.randint(0, 256, size=(H, W, elem_sz)).astype(np.uint8)
    noise = rng.randint(-10, 11, size=(H, W, elem_sz))
    noise[rng.rand(H, W) < 0.5] //= 3
    img = np.clip(img_prev.astype(np.int32) + noise, 0, 255).astype(np.uint8)
    for _ in range(max(1, H * W // 400)):
        y, x = rng.randint(0, H), rng.randint(0, W)
        img[y:y + 3, x:x + 4] = rng.randint(0, 256, size=img[y:y + 3, x:x + 4].shape)
    if elem_sz > 3:
        img[..., 3:] = rng.randint(0, 256, size=(H, W, elem_sz - 3))
    cur = (rng.randint(-64, 65, size=(H, W)) / 4.0).astype(np.float32)
    cur[rng.rand(H, W) < 0.3] += np.float32(0.1)
    prev = (cur + rng.uniform(-2.5, 2.5, size=(H, W))).astype(np.float32)
    r = rng.rand(H, W)
    prev[r < 0.1] = cur[r < 0.1]
    prev[(r >= 0.1) & (r < 0.15)] = cur[(r >= 0.1) & (r < 0.15)] + np.float32(1.5)  # df == thresh_disp where the sum is exact
    if nonfinite:
        for a in (cur, prev):
            r = rng.rand(H, W)
            a[r < 0.04] = np.nan
            a[(r >= 0.04) & (r < 0.07)] = np.inf
            a[(r >= 0.07) & (r < 0.10)] = -np.inf
    return cur, prev, img, img_prev


def _flat(H, W, elem_sz, level=100):
    """a flat image pair; bytes past the third differ wildly between the two (never read)"""
    a = np.full((H, W, elem_sz), level, np.uint8)
    b = a.copy()
    if elem_sz > 3:
        a[..., 3:] = 0
        b[..., 3:] = 255
    return a, b


def known_cases(elem_sz=3):
    """(name, cur, prev, img, img_prev, alpha, thresh_color, thresh_disp, want): the definition's corners, `want` written down by
    hand.  5 x 9 maps, cur = 2, prev = 3: a pixel that passes both gates at alpha = 0.5 becomes 2.5."""
    H, W = 5, 9
    f = np.float32
    cur, prev = np.full((H, W), 2, f), np.full((H, W), 3, f)
    cases = []

    def changed(y, x, delta):
        img, img_prev = _flat(H, W, elem_sz)
        img[y, x, :3] = np.array([100 + delta[0], 100 - delta[1], 100 + delta[2]], np.uint8)
        return img, img_prev

    def blocked(y0, y1, x0, x1):
        want = np.full((H, W), 2.5, f)
        want[y0:y1, x0:x1] = 2
        return want

    img, img_prev = changed(2, 4, (8, 8, 8))  # sad = 24 == thresh_color: every pixel passes
    cases.append(("m_equals_thresh_color", cur, prev, img, img_prev, 0.5, 24, 1.5, np.full((H, W), 2.5, f)))
    img, img_prev = changed(2, 4, (9, 8, 8))  # sad = 25 = thresh_color + 1: exactly the 3 x 3 pixels around (4, 2) keep cur
    cases.append(("one_pixel_blocks_its_3x3", cur, prev, img, img_prev, 0.5, 24, 1.5, blocked(1, 4, 3, 6)))
    cases.append(("thresh_color_0_static", cur, prev) + _flat(H, W, elem_sz) + (0.5, 0, 1.5, np.full((H, W), 2.5, f)))
    img, img_prev = _flat(H, W, elem_sz)  # the strongest change there is (sad = 765), in a corner: 2 x 2 pixels
    img[0, 0, :3], img_prev[0, 0, :3] = 255, 0
    cases.append(("corner_top_left", cur, prev, img, img_prev, 0.5, 764, 1.5, blocked(0, 2, 0, 2)))
    cases.append(("sad_765_passes_at_765", cur, prev, img, img_prev, 0.5, 765, 1.5, np.full((H, W), 2.5, f)))
    img, img_prev = changed(4, 8, (40, 0, 0))
    cases.append(("corner_bottom_right", cur, prev, img, img_prev, 0.5, 24, 1.5, blocked(3, 5, 7, 9)))
    img, img_prev = changed(0, 4, (0, 30, 0))
    cases.append(("edge_top", cur, prev, img, img_prev, 0.5, 24, 1.5, blocked(0, 2, 3, 6)))
    img, img_prev = changed(2, 0, (0, 0, 30))
    cases.append(("edge_left", cur, prev, img, img_prev, 0.5, 24, 1.5, blocked(1, 4, 0, 2)))
    # the disparity gate: df == thresh_disp passes, the next float above it does not, a NaN or an inf - inf never does
    p2 = prev.copy()
    p2[0, 0] = 3.5                                  # df = 1.5: passes, 2 + 0.5 * 1.5
    p2[0, 1] = np.nextafter(f(3.5), f(4))           # df just above 1.5
    p2[0, 2] = 0.5                                  # df = 1.5 from below: 2 + 0.5 * -1.5
    p2[0, 3] = np.nan
    p2[0, 4] = np.inf
    c2 = cur.copy()
    c2[1, 0] = np.nan
    c2[1, 1] = np.inf
    p2[1, 1] = np.inf                               # inf - inf = NaN
    want = np.full((H, W), 2.5, f)
    want[0, :5] = [2.75, 2, 1.25, 2, 2]
    want[1, 0] = np.nan
    want[1, 1] = np.inf
    cases.append(("disparity_gate", c2, p2) + _flat(H, W, elem_sz) + (0.5, 24, 1.5, want))
    # thresh_disp = +inf: an infinite t passes and behaves as the lines say
    want = np.full((H, W), 2.5, f)
    want[0, :5] = [2.75, 0.5 * float(p2[0, 1]) + 1.0, 1.25, 2, np.inf]  # (a NaN never passes: NaN <= inf is false)
    want[1, 0] = np.nan
    want[1, 1] = np.inf                             # the gate fails on NaN <= inf: out = c = inf
    cases.append(("thresh_disp_inf", c2, p2) + _flat(H, W, elem_sz) + (0.5, 24, np.inf, want))
    # alpha = 0 and alpha = 1 on finite maps (dyadic values a factor of two apart at the most: q - c and c + t are exact)
    rng = np.random.RandomState(5)
    c3 = (rng.randint(64, 128, size=(H, W)) / 64.0).astype(f)
    q3 = (rng.randint(64, 128, size=(H, W)) / 64.0).astype(f)
    cases.append(("alpha_0_gives_cur", c3, q3) + _flat(H, W, elem_sz) + (0.0, 24, 1.5, c3.copy()))
    cases.append(("alpha_1_gives_prev", c3, q3) + _flat(H, W, elem_sz) + (1.0, 24, 1.5, q3.copy()))
    return cases


KNOWN_IDS = [c[0] for c in known_cases()]


def seam_case(side):
    """Two side-by-side frames [6][2 * 7][3] for the seam of the halves.  side = 'left': the right half changes strongly at its
    column 0 between the frames while the left half is static, so the left view's column W - 1 must be filtered although its
    neighbour in the buffer moved; side = 'right': the mirror case, the left half's column W - 1 changes, the right view's
    column 0 must be filtered.  Returns (sbs_prev, sbs, view index that must be filtered everywhere)."""
    H, W = 6, 7
    prev = np.full((H, 2 * W, 3), 90, np.uint8)
    cur = prev.copy()
    if side == "left":
        cur[:, W] = 250
        return prev, cur, 0
    cur[:, W - 1] = 250
    return prev, cur, 1


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("elem_sz", [3, 4])
def test_known_answers(elem_sz):
    for name, cur, prev, img, img_prev, alpha, tc, td, want in known_cases(elem_sz):
        keep = cur.copy()
        got = temporal_ref(cur, prev, img, img_prev, alpha, tc, td)
        assert np.array_equal(got, want, equal_nan=True), name
        assert np.array_equal(temporal_loop(cur, prev, img, img_prev, alpha, tc, td), want, equal_nan=True), name
        assert np.array_equal(cur, keep, equal_nan=True)


@pytest.mark.parametrize("shape", SHAPES[:6], ids=SHAPE_IDS[:6])
def test_vectorised_form_is_the_scalar_loop(shape):
    H, W = shape
    for elem_sz, params in ((3, (ALPHA, THRESH_COLOR, THRESH_DISP)), (4, (0.25, 9, np.inf)), (3, (1.0, 40, 0.0))):
        cur, prev, img, img_prev = temporal_case(H * 31 + W + elem_sz, H, W, elem_sz)
        got = temporal_ref(cur, prev, img, img_prev, *params)
        assert got.dtype == np.float32 and np.array_equal(got, temporal_loop(cur, prev, img, img_prev, *params), equal_nan=True)
        if H * W >= 300:
            m = sad_max(img, img_prev)
            assert (m <= params[1]).any() and (m > params[1]).any()          # both sides of the colour gate
            assert np.isnan(got).any() and np.isinf(got).any()
            same = np.array_equal(got, cur, equal_nan=True)
            assert not same or params[2] == 0.0


def test_seam_cases_filter_the_static_half():
    for side in ("left", "right"):
        sbs_prev, sbs, static = seam_case(side)
        cur = np.full((6, 7), 2, np.float32)
        prev = np.full((6, 7), 3, np.float32)
        now, before = halves(sbs), halves(sbs_prev)
        out = [temporal_ref(cur, prev, now[v], before[v]) for v in (0, 1)]
        assert np.all(out[static] == 2.5)
        moved = out[1 - static]
        col = 0 if static == 0 else 6
        assert np.all(moved[:, col] == 2) and np.all(moved[:, 3] == 2.5)


# ----------------------------------------------------------------------------- on the oracle chain
SEQ = dict(H=40, W=72, D=8, zd=4, usd=9, lsd=4)


def _chain_maps(orc, sbs, p):
    dl, dr, _, _ = interp_frame(orc, sbs, p, 2, False)
    return dl, dr


def static_noisy_sequence(n=6):
    """One synthetic frame, n times, each with independent seeded noise in {-2 .. 2} per channel"""
    from stm_amd import synth
    s = SEQ
    base, off = synth.sbs_frame(s["H"], s["W"], s["D"], s["zd"])
    rng = np.random.RandomState(20261)
    frames = [np.clip(base.astype(np.int32) + rng.randint(-2, 3, size=base.shape), 0, 255).astype(np.uint8) for _ in range(n)]
    return frames, off


def moving_rectangle_sequence(n=3):
    """The same frame with a flat rectangle that moves 8 px per frame over both halves"""
    from stm_amd import synth
    s = SEQ
    base, _ = synth.sbs_frame(s["H"], s["W"], s["D"], s["zd"])
    frames = []
    for k in range(n):
        f = base.copy()
        for x0 in (6 + 8 * k, s["W"] + 4 + 8 * k):
            f[10:24, x0:x0 + 14] = (200, 60, 30)
        frames.append(f)
    return frames


def mixed_sequence(n, seed=77):
    """moving_rectangle_sequence under the noise of static_noisy_sequence: pixels on both sides of both gates in every frame"""
    rng = np.random.RandomState(seed)
    return [np.clip(f.astype(np.int32) + rng.randint(-2, 3, size=f.shape), 0, 255).astype(np.uint8) for f in moving_rectangle_sequence(n)]


def test_static_noisy_scene_flickers_less(orc):
    """40 x 72, D = 8, six frames of one scene under +-2 noise, left and right maps together.  Mean |out_k - out_(k-1)| over
    k >= 1 falls with the step (measured 0.0110 -> 0.0049 px), and the mean |disp_l - true offset| does not suffer (0.1717
    without, 0.1716 with): only the direction is asserted.  The test prints the four figures; larger scenes: DESIGN.md section 13."""
    s = SEQ
    p = _P(s["D"], s["zd"], usd=s["usd"], lsd=s["lsd"])
    frames, off = static_noisy_sequence()
    for k in range(1, len(frames)):  # every pixel satisfies the colour gate by construction
        assert sad_map(frames[k], frames[k - 1]).max() <= 12
        for v in (0, 1):
            assert sad_max(halves(frames[k])[v], halves(frames[k - 1])[v]).max() <= 12 < THRESH_COLOR
    maps = [_chain_maps(orc, f, p) for f in frames]
    out = temporal_recursion(frames, maps)

    def flicker(seq):
        return float(np.mean([np.mean(np.abs(np.stack(seq[k]) - np.stack(seq[k - 1]))) for k in range(1, len(seq))]))

    def err(seq):
        return float(np.mean([np.mean(np.abs(m[0] - off)) for m in seq[1:]]))

    raw, stab = flicker(maps), flicker(out)
    print("static noisy scene: mean |out_k - out_(k-1)| %.4f without the step, %.4f with it; mean |disp_l - truth| %.4f without, %.4f with"
          % (raw, stab, err(maps), err(out)))
    assert raw > 0, "the noise never changed a map: the scene shows nothing"
    assert stab < raw, (stab, raw)


def test_moving_rectangle_is_left_alone(orc):
    """Every pixel whose 3 x 3 colour change exceeds the gate keeps this frame's value bit for bit; elsewhere something is blended"""
    s = SEQ
    p = _P(s["D"], s["zd"], usd=s["usd"], lsd=s["lsd"])
    frames = moving_rectangle_sequence()
    maps = [_chain_maps(orc, f, p) for f in frames]
    out = temporal_recursion(frames, maps)
    blocked = blended = 0
    for k in range(1, len(frames)):
        for v in (0, 1):
            m = sad_max(halves(frames[k])[v], halves(frames[k - 1])[v])
            moved = m > THRESH_COLOR
            assert moved.any() and not moved.all()
            assert np.array_equal(out[k][v][moved], maps[k][v][moved])
            assert np.array_equal(out[k][v][~moved], temporal_ref(maps[k][v], out[k - 1][v], halves(frames[k])[v],
                                                                  halves(frames[k - 1])[v])[~moved])
            blocked += int(moved.sum())
            blended += int((out[k][v] != maps[k][v]).sum())
    assert blocked > 0 and blended > 0
