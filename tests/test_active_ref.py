"""The active picture area's numpy statement (stm_active_detect, stm_active_fill, stm_depth_fit_rect, stm_overlay_fit_rect in
include/stm_hip.h), its known answers, its sequences, and what it buys on the oracle's maps of the committed bud pair.  No GPU:
tests/test_gpu_active.py compares the kernels with these functions."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_depth_ref import depth_fit_ref
from test_overlay_fit_ref import _update, alpha_box_ref, fit_bins_ref, footprint_ref, overlay_fit_ref, state_disparity_ref

f32 = np.float32
STATE_WORDS = 16
DEFAULTS = dict(thresh_luma=24, lit_permille=10, max_bar_permille=300, hold=12)  # stm_set_active_auto's, video.ACTIVE_AUTO_DEFAULT


# ----------------------------------------------------------------------------- the definition
def counts_ref(img, thresh_luma):
    """steps 1 - 2: the lit pixels per row, then per column, H + W counts"""
    p = np.asarray(img)[:, :, :3].astype(np.int64)
    lit = ((p[:, :, 0] + 2 * p[:, :, 1] + p[:, :, 2]) >> 2) > thresh_luma
    return np.concatenate([lit.sum(axis=1), lit.sum(axis=0)]).astype(np.int64)


def bars_ref(counts, H, W, lit_permille, max_bar_permille):
    """steps 3 - 4: m[0 .. 3] (top, bottom, left, right), capped, or None for a blank frame"""
    rows = np.nonzero(counts[:H] * 1000 > lit_permille * W)[0]
    cols = np.nonzero(counts[H:] * 1000 > lit_permille * H)[0]
    if rows.size == 0 or cols.size == 0:
        return None
    cap_y, cap_x = H * max_bar_permille // 1000, W * max_bar_permille // 1000
    return [min(int(rows[0]), cap_y), min(H - 1 - int(rows[-1]), cap_y), min(int(cols[0]), cap_x), min(W - 1 - int(cols[-1]), cap_x)]


def decide_ref(counts, H, W, state, lit_permille, max_bar_permille, hold, restart=False, cut_flag=0):
    """steps 3 - 7 on the counts: the new state (int32, 16)"""
    old = np.asarray(state, np.int32)
    assert old.shape == (STATE_WORDS,)
    history = old[0] != 0 and old[6] == H and old[7] == W
    restart = (not history) or bool(restart) or cut_flag == 1
    m = bars_ref(counts, H, W, lit_permille, max_bar_permille)
    if m is None:
        if not restart:
            out = old.copy()
            out[5] = 0
            return out
        return np.array([0, 0, H, 0, W, 0, H, W] + [0] * 8, np.int32)
    was = [int(old[1]), int(old[2]), int(old[3]), int(old[4])] if history else [0, H, 0, W]
    B = [was[0], H - was[1], was[2], W - was[3]]
    cand, run = [int(v) for v in old[8:12]], [int(v) for v in old[12:16]]
    for i in range(4):
        b = m[i]
        if restart:
            B[i], cand[i], run[i] = b, b, 0
        elif b < B[i]:
            B[i], run[i] = b, 0
        elif b == B[i]:
            run[i] = 0
        else:
            cand[i] = b if run[i] == 0 else min(cand[i], b)
            run[i] += 1
            if run[i] >= hold:
                B[i], run[i] = cand[i], 0
    now = [B[0], H - B[1], B[2], W - B[3]]
    return np.array([1] + now + [int(now != was), H, W] + cand + run, np.int32)


def detect_ref(img, state=None, thresh_luma=24, lit_permille=10, max_bar_permille=300, hold=12, restart=False, cut_flag=0):
    """stm_active_detect on an image [H][W][>= 3]; None = a zeroed state.  Returns (state, counts)."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    st = np.zeros(STATE_WORDS, np.int32) if state is None else state
    c = counts_ref(img, thresh_luma)
    return decide_ref(c, H, W, st, lit_permille, max_bar_permille, hold, restart, cut_flag), c


def rect_of(state):
    return tuple(int(v) for v in np.asarray(state)[1:5])


def fill_ref(disp, rect, value):
    """stm_active_fill: `value` outside rows [top, bottom) x columns [left, right), the inside bit for bit; None = the map"""
    out = np.array(disp, f32)
    if rect is None:
        return out
    t, b, l, r = rect
    keep = out[t:b, l:r].copy()
    out[...] = f32(value)
    out[t:b, l:r] = keep
    return out


def depth_fit_rect_ref(dl, dr, disp_lo, disp_hi, max_gain, clip_permille, rate, state, rect):
    """stm_depth_fit_rect: stm_depth_fit on the pixels of both maps inside the rectangle"""
    if rect is None:
        return depth_fit_ref(dl, dr, disp_lo, disp_hi, max_gain, clip_permille, rate, state)
    t, b, l, r = rect
    return depth_fit_ref(np.asarray(dl, f32)[t:b, l:r], np.asarray(dr, f32)[t:b, l:r], disp_lo, disp_hi, max_gain, clip_permille, rate, state)


def slide_ref(a, b, A, B):
    """the footprint's interval [a, b) of one axis moved into the active interval [A, B)"""
    lo, hi = max(a, A), min(b, B)
    if lo < hi:
        return lo, hi
    n = min(b - a, B - A)
    return (A, A + n) if b <= A else (B - n, B)


def overlay_fit_rect_ref(dl, dr, overlay, x0, y0, Hv, Wv, rect, gain=1.0, conv=0.0, near_permille=20, margin=1.0, pad=8, limit_lo=-4096.0,
                         limit_hi=4096.0, rate_near=1.0, rate_far=0.1, restart=False, state=None, cut_flag=0):
    """stm_overlay_fit_rect: stm_overlay_fit with the map rectangle of step 2 slid into the active one"""
    kw = dict(gain=gain, conv=conv, near_permille=near_permille, margin=margin, pad=pad, limit_lo=limit_lo, limit_hi=limit_hi,
              rate_near=rate_near, rate_far=rate_far, restart=restart, state=state, cut_flag=cut_flag)
    if rect is None:
        return overlay_fit_ref(dl, dr, overlay, x0, y0, Hv, Wv, **kw)
    state = np.zeros(4, f32) if state is None else np.array(state, f32)
    dl, dr = np.asarray(dl, f32), np.asarray(dr, f32)
    H, W = dl.shape
    fp = footprint_ref(alpha_box_ref(overlay), int(x0), int(y0), int(pad), Hv, Wv, H, W)
    if fp is None:
        return state
    my0, my1 = slide_ref(fp[0], fp[1], rect[0], rect[1])
    mx0, mx1 = slide_ref(fp[2], fp[3], rect[2], rect[3])
    b = np.concatenate([fit_bins_ref(dl[my0:my1, mx0:mx1]), fit_bins_ref(dr[my0:my1, mx0:mx1])])
    n = int(b.size)
    if n == 0:
        return state
    k = n * int(near_permille) // 1000
    lo = int(np.argmax(np.cumsum(np.bincount(b, minlength=4096)) > k))
    return _update(state, lo, gain, conv, Wv, W, margin, limit_lo, limit_hi, rate_near, rate_far, bool(restart) or cut_flag == 1)


# ----------------------------------------------------------------------------- pictures with bars
def bud():
    import stm_amd
    return tuple(stm_amd.bmp_io.read_bmp(os.path.join(GOLDEN, f)) for f in ("bud_2.bmp", "bud_3.bmp"))


def paint_bars(img, top=0, bottom=0, left=0, right=0, level=0, noise=0, seed=0):
    """the bars painted over the picture: `level` plus uniform noise in [-noise, +noise] (level 0: [0, noise]), each byte on its own"""
    out = np.array(img, np.uint8)
    H, W = out.shape[:2]
    rng = np.random.RandomState(seed)
    mask = np.zeros((H, W), bool)
    mask[:top] = mask[H - bottom:] = True
    mask[:, :left] = True
    mask[:, W - right:] = True
    lo = max(level - noise, 0)
    v = rng.randint(lo, level + noise + 1, size=out.shape).astype(np.uint8)
    out[mask] = v[mask]
    return out


def frame_with(H, W, top, bottom, left, right, seed=0, dark=8):
    """a bright noise picture inside dark bars (levels 0 .. dark)"""
    rng = np.random.RandomState(seed)
    img = rng.randint(0, dark + 1, size=(H, W, 3)).astype(np.uint8)
    img[top:H - bottom, left:W - right] = rng.randint(60, 256, size=(H - top - bottom, W - left - right, 3))
    return img


# ----------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("thresh", [24, 32])
def test_letterbox_and_pillarbox_of_the_bud_frame(stm, thresh):
    L, _ = bud()
    H, W = L.shape[:2]
    assert (H, W) == (384, 640)
    kw = dict(DEFAULTS, thresh_luma=thresh)
    for level, noise in ((0, 0), (16, 2), (0, 3)):
        st, _ = detect_ref(paint_bars(L, top=49, bottom=49, level=level, noise=noise, seed=1), None, **kw)
        assert rect_of(st) == (49, 335, 0, 640) and st[0] == 1 and st[5] == 1, (level, noise)
    st, _ = detect_ref(paint_bars(L, left=80, right=80), None, **kw)
    assert rect_of(st) == (0, 384, 80, 560)
    st, _ = detect_ref(L, None, **kw)
    assert rect_of(st) == (0, 384, 0, 640) and st[5] == 0  # no bars: the rectangle is the frame, nothing changed


def test_limited_range_black_needs_the_default_threshold(stm):
    """bars at 16 +- 2 are found at 24 and missed at 16: the reason for the default"""
    L, _ = bud()
    img = paint_bars(L, top=49, bottom=49, level=16, noise=2, seed=1)
    assert rect_of(detect_ref(img, None, **DEFAULTS)[0]) == (49, 335, 0, 640)
    assert rect_of(detect_ref(img, None, **dict(DEFAULTS, thresh_luma=16))[0]) != (49, 335, 0, 640)


def test_a_logo_in_a_bar_does_not_move_it():
    """fewer lit pixels per line than the permille rule: 6 of 640 columns and 3 of 384 rows at 10 permille"""
    H, W = 384, 640
    img = frame_with(H, W, 49, 49, 0, 0, seed=2)
    img[10:13, 600:606] = 255  # rows: 6 * 1000 <= 10 * 640; columns 600 .. 605 are picture columns anyway
    assert rect_of(detect_ref(img, None, **DEFAULTS)[0]) == (49, 335, 0, 640)
    img[10:13, 600:607] = 255  # 7 lit pixels: 7000 > 6400, the rows are picture
    assert rect_of(detect_ref(img, None, **DEFAULTS)[0]) == (10, 335, 0, 640)
    side = frame_with(H, W, 0, 0, 80, 80, seed=3)
    side[100:103, 20:40] = 255  # 3 rows of 384: 3000 <= 3840, the columns stay bar
    assert rect_of(detect_ref(side, None, **DEFAULTS)[0]) == (0, 384, 80, 560)
    side[100:104, 20:40] = 255  # 4 rows: 4000 > 3840
    assert rect_of(detect_ref(side, None, **DEFAULTS)[0]) == (0, 384, 20, 560)


def test_counts():
    img = np.zeros((5, 7, 3), np.uint8)
    img[1, 2] = (0, 50, 0)   # Y = 25: lit at 24
    img[3, 2] = (48, 24, 0)  # Y = 24: not lit
    img[4, 6] = (255, 255, 255)
    c = counts_ref(img, 24)
    assert c.tolist() == [0, 1, 0, 0, 1] + [0, 0, 1, 0, 0, 0, 1]


def test_the_cap():
    """a lit centre in a dark frame: at most max_bar_permille a side, floor division"""
    H, W = 100, 210
    img = frame_with(H, W, 45, 45, 100, 100, seed=4)
    assert rect_of(detect_ref(img, None, **DEFAULTS)[0]) == (30, 70, 63, 147)
    assert rect_of(detect_ref(img, None, **dict(DEFAULTS, max_bar_permille=450))[0]) == (45, 55, 94, 116)  # 210 * 450 // 1000 = 94
    assert rect_of(detect_ref(img, None, **dict(DEFAULTS, max_bar_permille=0))[0]) == (0, 100, 0, 210)


# ----------------------------------------------------------------------------- sequences
SEQ_H, SEQ_W = 40, 64


def seq_frame(top, bottom=0, left=0, right=0, seed=0):
    return frame_with(SEQ_H, SEQ_W, top, bottom, left, right, seed=seed)


def run_sequence(frames, detect, hold=3, **kw):
    """the states after each of `frames` = [(image, restart, cut_flag)], through detect(img, state, restart, cut_flag) -> state"""
    st, out = np.zeros(STATE_WORDS, np.int32), []
    for img, restart, cut_flag in frames:
        st = detect(img, st, restart, cut_flag)
        out.append(np.array(st))
    return out


def ref_step(hold):
    def step(img, st, restart, cut_flag):
        return detect_ref(img, st, 24, 10, 300, hold, restart, cut_flag)[0]
    return step


def growth_sequence():
    """no bar; then 6, 8, 5 rows of top bar (grows at the third, to the least); a lit frame; then 5, 5, 5 again"""
    tops = [0, 6, 8, 5, 5, 2, 5, 5, 5, 5]
    return [(seq_frame(t, seed=i), False, 0) for i, t in enumerate(tops)]


def test_a_bar_grows_at_the_hold_th_agreeing_frame_to_the_least_of_the_run():
    got = [rect_of(s)[0] for s in run_sequence(growth_sequence(), ref_step(3))]
    #       0  6  8  5  5  2  5  5  5  5
    assert got == [0, 0, 0, 5, 5, 2, 2, 2, 5, 5]
    changed = [int(s[5]) for s in run_sequence(growth_sequence(), ref_step(3))]
    assert changed == [0, 0, 0, 1, 0, 1, 0, 0, 1, 0]


def test_a_lit_frame_inside_the_run_restarts_it():
    """b == B in the middle of a run sets run = 0: the two frames before do not count towards the hold"""
    tops = [0, 6, 6, 0, 6, 6, 6]
    states = run_sequence([(seq_frame(t, seed=i), False, 0) for i, t in enumerate(tops)], ref_step(3))
    assert [rect_of(s)[0] for s in states] == [0, 0, 0, 0, 0, 0, 6]
    assert [int(s[12]) for s in states] == [0, 1, 2, 0, 1, 2, 0]


def test_hold_1_takes_every_frame_on_its_own():
    tops = [0, 6, 8, 5, 0, 7]
    states = run_sequence([(seq_frame(t, seed=i), False, 0) for i, t in enumerate(tops)], ref_step(1))
    assert [rect_of(s)[0] for s in states] == tops


def test_each_side_on_its_own():
    frames = [(seq_frame(0, seed=0), False, 0), (seq_frame(4, 6, 10, 12, seed=1), False, 0), (seq_frame(4, 0, 10, 14, seed=2), False, 0),
              (seq_frame(4, 6, 9, 12, seed=3), False, 0)]
    states = run_sequence(frames, ref_step(2))
    assert [rect_of(s) for s in states] == [(0, 40, 0, 64), (0, 40, 0, 64), (4, 40, 10, 52), (4, 40, 9, 52)]
    assert states[3][12:16].tolist() == [0, 1, 0, 0]  # the bottom bar's run started again at frame 3


def blank():
    return np.zeros((SEQ_H, SEQ_W, 3), np.uint8)


def test_blank_frames():
    # with history: only `changed` is written
    st = run_sequence([(seq_frame(5, seed=0), False, 0), (seq_frame(9, seed=1), False, 0)], ref_step(4))[-1]
    assert rect_of(st) == (5, 40, 0, 64) and st[12] == 1 and st[5] == 0
    st[5] = 1
    after = detect_ref(blank(), st, 24, 10, 300, 4)[0]
    want = st.copy()
    want[5] = 0
    assert np.array_equal(after, want)
    # without: bars off, nothing known, and the next frame that is not blank starts afresh
    none = detect_ref(blank(), None, 24, 10, 300, 4)[0]
    assert none.tolist() == [0, 0, SEQ_H, 0, SEQ_W, 0, SEQ_H, SEQ_W] + [0] * 8
    assert rect_of(detect_ref(seq_frame(7, seed=2), none, 24, 10, 300, 4)[0]) == (7, 40, 0, 64)
    # a blank frame on a restart drops the history too
    assert np.array_equal(detect_ref(blank(), st, 24, 10, 300, 4, restart=True)[0], none)
    assert np.array_equal(detect_ref(blank(), st, 24, 10, 300, 4, cut_flag=1)[0], none)


def test_restart_by_the_argument_and_by_the_cut_flag():
    st = run_sequence([(seq_frame(0, seed=0), False, 0)], ref_step(5))[-1]
    img = seq_frame(6, 3, seed=1)
    assert rect_of(detect_ref(img, st, 24, 10, 300, 5)[0]) == (0, 40, 0, 64)  # held
    for kw in (dict(restart=True), dict(cut_flag=1)):
        got = detect_ref(img, st, 24, 10, 300, 5, **kw)[0]
        assert got.tolist() == [1, 6, 37, 0, 64, 1, SEQ_H, SEQ_W, 6, 3, 0, 0, 0, 0, 0, 0], kw
    assert rect_of(detect_ref(img, st, 24, 10, 300, 5, cut_flag=0)[0]) == (0, 40, 0, 64)


def test_a_state_of_another_size_is_no_history():
    st = run_sequence([(seq_frame(5, seed=0), False, 0)], ref_step(5))[-1]
    other = frame_with(SEQ_H, SEQ_W + 1, 9, 0, 0, 0, seed=1)
    got = detect_ref(other, st, 24, 10, 300, 5)[0]
    assert rect_of(got) == (9, SEQ_H, 0, SEQ_W + 1) and got[6:8].tolist() == [SEQ_H, SEQ_W + 1]
    assert got[5] == 1  # against the whole frame, not against the other size's rectangle


# ----------------------------------------------------------------------------- the consumers
def test_fill():
    d = np.arange(30, dtype=f32).reshape(5, 6)
    d[2, 3] = np.nan
    out = fill_ref(d, (1, 4, 2, 5), -7.5)
    assert out[1:4, 2:5].tobytes() == d[1:4, 2:5].tobytes()
    mask = np.ones((5, 6), bool)
    mask[1:4, 2:5] = False
    assert (out[mask] == f32(-7.5)).all()
    assert fill_ref(d, (0, 5, 0, 6), 3).tobytes() == d.tobytes() and fill_ref(d, None, 3).tobytes() == d.tobytes()


def test_slide_rule():
    assert slide_ref(10, 20, 5, 30) == (10, 20)     # inside
    assert slide_ref(10, 20, 15, 30) == (15, 20)    # intersecting
    assert slide_ref(2, 8, 10, 30) == (10, 16)      # wholly above: the first lines of the picture
    assert slide_ref(32, 38, 10, 30) == (24, 30)    # wholly below: the last
    assert slide_ref(30, 38, 10, 30) == (22, 30)    # touching is not intersecting
    assert slide_ref(40, 90, 10, 30) == (10, 30)    # longer than the active interval
    assert slide_ref(0, 10, 10, 12) == (10, 12)
    assert slide_ref(0, 50, 10, 30) == (10, 30)     # covering


def test_depth_fit_rect_counts_only_the_rectangle():
    dl = np.full((20, 30), 2.0, f32)
    dr = np.full((20, 30), -2.0, f32)
    dl[:4], dr[16:] = -16.0, 12.0  # bars
    z = np.zeros(4, f32)
    whole = depth_fit_ref(dl, dr, -4, 4, 1.0, 0, 1.0, z)
    inside = depth_fit_rect_ref(dl, dr, -4, 4, 1.0, 0, 1.0, z, (4, 16, 0, 30))
    assert float(whole[1]) == pytest.approx(8 / 28) and float(inside[1]) == 1.0
    assert depth_fit_rect_ref(dl, dr, -4, 4, 1.0, 0, 1.0, z, None).tobytes() == whole.tobytes()


def test_overlay_fit_rect_places_a_strip_in_the_bar_by_the_nearest_picture_rows():
    H, W = 40, 60
    dl = np.full((H, W), 5.0, f32)
    dl[30:34] = -3.0   # the last picture rows
    dl[34:] = -16.0    # the bottom bar
    dr = dl.copy()
    ov = np.full((4, 20, 4), 255, np.uint8)
    kw = dict(near_permille=0, margin=0.0, pad=0)
    assert float(overlay_fit_ref(dl, dr, ov, 10, 35, H, W, **kw)[1]) == -16.0
    assert float(overlay_fit_rect_ref(dl, dr, ov, 10, 35, H, W, (6, 34, 0, W), **kw)[1]) == -3.0
    assert float(overlay_fit_rect_ref(dl, dr, ov, 10, 1, H, W, (6, 34, 0, W), **kw)[1]) == 5.0  # in the top bar: rows 6 .. 9
    assert overlay_fit_rect_ref(dl, dr, ov, 10, 35, H, W, None, **kw).tobytes() == overlay_fit_ref(dl, dr, ov, 10, 35, H, W, **kw).tobytes()


# ----------------------------------------------------------------------------- the effect on the oracle's maps
P = dict(D=32, zd=16, ad=10.0, ce=30.0, ucd=6.0, lcd=20.0, usd=17, lsd=8, ts=20, th=0.4, N=8, angle=18.43)  # make_golden_c1.py's
BUDGET = dict(disp_lo=-4.0, disp_hi=4.0, max_gain=1.0, clip_permille=20)
OVERLAY_LIMITS = (-8.0, 10.0)  # a panel's comfortable range: what black bars match at (-zero_disp = -16, smeared to -9) lies beyond it
STRIP_ROWS = 24


def oracle_maps(orc, L, R):
    H, W, _ = L.shape
    sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
    o = orc.adcensus_stm(sbs, H, W, P["N"], P["angle"], P["D"], P["zd"], P["ad"], P["ce"], P["ucd"], P["lcd"], P["usd"], P["lsd"], P["ts"], P["th"])
    return o["disp_l"], o["disp_r"]


def gain_of(dl, dr, rect):
    return float(depth_fit_rect_ref(dl, dr, BUDGET["disp_lo"], BUDGET["disp_hi"], BUDGET["max_gain"], BUDGET["clip_permille"], 1.0,
                                    np.zeros(4, f32), rect)[1])


def effect(orc):
    """the numbers of tools/active_effect.py: per case the measured rectangle and the three gains, and the overlay's placements"""
    L, R = bud()
    H, W = L.shape[:2]
    plain = oracle_maps(orc, L, R)
    cases = {"letterbox_noise": dict(top=49, bottom=49, level=0, noise=3), "pillarbox_black": dict(left=80, right=80)}
    res = {}
    for name, bars in cases.items():
        bl, br = paint_bars(L, seed=11, **bars), paint_bars(R, seed=12, **bars)  # noise independent in the two eyes
        rect = rect_of(detect_ref(bl, None, **DEFAULTS)[0])
        maps = oracle_maps(orc, bl, br)
        res[name] = {"rect": list(rect), "gain_rect": gain_of(*maps, rect), "gain_whole": gain_of(*maps, None),
                     "gain_unbarred_rect": gain_of(*plain, rect)}
    # a subtitle strip wholly inside the bottom bar of a pure black letterbox
    bl, br = paint_bars(L, top=49, bottom=49), paint_bars(R, top=49, bottom=49)
    rect = rect_of(detect_ref(bl, None, **DEFAULTS)[0])
    maps = oracle_maps(orc, bl, br)
    ov = np.zeros((STRIP_ROWS, W, 4), np.uint8)
    ov[:, W // 3:2 * W // 3] = 255
    y0 = rect[1] + 8  # rows 343 .. 366 of the bar 335 .. 383
    kw = dict(near_permille=20, margin=1.0, pad=0, limit_lo=OVERLAY_LIMITS[0], limit_hi=OVERLAY_LIMITS[1])
    without = overlay_fit_ref(*maps, ov, 0, y0, H, W, **kw)
    under = overlay_fit_rect_ref(*maps, ov, 0, y0, H, W, rect, **kw)
    slid = overlay_fit_ref(*plain, ov, 0, rect[1] - STRIP_ROWS, H, W, **kw)
    res["overlay_in_bottom_bar"] = {"rect": list(rect), "y0": y0, "limits": list(OVERLAY_LIMITS),
                                    "without_rect": state_disparity_ref(without, *OVERLAY_LIMITS), "nearest_without_rect": float(without[2]),
                                    "with_rect": state_disparity_ref(under, *OVERLAY_LIMITS),
                                    "unbarred_slid": state_disparity_ref(slid, *OVERLAY_LIMITS)}
    return res


@pytest.fixture(scope="module")
def effect_numbers(orc, stm):
    return effect(orc)


@pytest.mark.parametrize("case,want", [("letterbox_noise", (49, 335, 0, 640)), ("pillarbox_black", (0, 384, 80, 560))])
def test_the_rectangle_restores_the_depth_budget(effect_numbers, case, want):
    """the gain fitted under the measured rectangle lies within 10 % of the unbarred pair's over the same rectangle; the gain fitted
    on the whole maps is more than 25 % away from it"""
    e = effect_numbers[case]
    print(case, e)
    assert tuple(e["rect"]) == want
    ref = e["gain_unbarred_rect"]
    assert abs(e["gain_rect"] - ref) <= 0.10 * ref
    assert abs(e["gain_whole"] - ref) > 0.25 * ref


def test_a_subtitle_in_the_bottom_bar_is_placed_by_the_picture(effect_numbers):
    e = effect_numbers["overlay_in_bottom_bar"]
    print(e)
    assert e["without_rect"] == OVERLAY_LIMITS[0]
    assert abs(e["with_rect"] - e["unbarred_slid"]) <= 1.0
