"""The vertical kernel of the frame's fast path (stm_k_pq_v12r: exact windows as runs of vector adds, one column per wave) against
the CPU oracle's chain and against the masked-MFMA column kernel it replaced as the default (stm_k_pq_v12m, stm_set_agg_variant(800)).

The volume after both vertical passes, all 2 D H W floats, is compared byte for byte with the oracle's, the maps with the oracle's,
and both with what the MFMA variant leaves.  Shapes are the smallest at which the kernel can go wrong.  It keeps the last N = 72 rows
of either pass in registers, input row r in slot (r - 36) mod N and first-pass row r in slot r mod N, reads its input sixteen rows
ahead and runs the second pass 36 rows behind the first: heights below the read-ahead, one past sixteen, around N and beyond two
turns of the rings, and heights at which a column is cut into two and three row ranges; one column, one group of four, ragged widths; a record with padding hypotheses; the three arm limits the fast
path takes.  Every case first asserts on the oracle's arms that it holds the window lengths it is there for."""
import numpy as np
import pytest

import agg_tap_cases as tc
import test_gpu_agg_tap as tap

pytestmark = pytest.mark.gpu

N = 72    # rows of a ring (VA_RING, csrc/stm_hwin.h)
LAG = 36  # the input ring's slot of row r is (r - LAG) mod N (VA_LAG)
MFMA = tap.Form("mfma_column_px2", 800)  # stm_k_pq_hc2, stm_k_pq_v12m, stm_k_pq_hsr on PX order 2: every answer is the default's


def _pair(content, H, W, p):
    """(left, right) uint8 [H][W][3], read only.  flat: one colour (every arm runs to usd or the border); noise: independent
    uniform pixels (arms stop at their first steps: no window is longer than 4 rows)"""
    if content in ("synth", "mondrian"):
        return tap._pair(content, H, W, p)
    key = ("pair", content, H, W)
    if key not in tap._CACHE:
        if content == "flat":
            pair = np.full((H, W, 3), 97, np.uint8), np.full((H, W, 3), 97, np.uint8)
        else:
            rng = np.random.RandomState(5)
            pair = rng.randint(0, 256, (H, W, 3)).astype(np.uint8), rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        for a in pair:
            a.setflags(write=False)
        tap._CACHE[key] = pair
    return tap._CACHE[key]


def _windows(cross):
    """first row and length of every pixel's vertical window [y - armU, y + armD) of one view"""
    up, down = cross[0].astype(np.int64), cross[1].astype(np.int64)
    y = np.arange(up.shape[0])[:, None]
    return y - up, up + down


def _crosses(first, length, phase):
    """pixels whose window holds rows r - 1 and r with (r - phase) % N == 0: its sum passes the end of a ring"""
    k = -((phase - first) // N)  # the smallest k with phase + k N >= first
    r = phase + k * N
    return (length > 0) & (r > first) & (r < first + length)


def _assert_holds(wants, crosses, usd, H, W):
    first, length = zip(*[_windows(c) for c in crosses])
    first, length = np.stack(first), np.stack(length)
    assert length.min() >= 0 and length.max() <= 2 * usd <= N
    for w in wants:
        if w == "empty":
            assert (length == 0).any(), "no empty window"
        elif w == "short":
            assert ((length >= 1) & (length <= 3)).any(), "no window of 1 to 3 rows"
        elif w == "only_short":
            assert length.max() <= 4, "longest window %d" % length.max()
        elif w == "full":
            assert (length == 2 * usd).any(), "no window of 2 usd rows"
        elif w == "full_count":
            assert int((length[0] == 2 * usd).sum()) == (H - 2 * usd) * W
        elif w == "clipped":
            assert ((length > usd) & (length < 2 * usd)).any(), "no window clipped by a border"
        elif w == "column":
            assert H - 1 <= usd and (length == H - 1).all(), "a window that is not the column without its last row"
        elif w == "between":
            assert len(np.unique(length)) >= min(H, 20) // 2, "only %d different lengths" % len(np.unique(length))
        elif w == "wrap_in":
            assert _crosses(first, length, LAG).any(), "no window across the end of the input ring"
        elif w == "wrap_mid":
            assert _crosses(first, length, 0).any(), "no window across the end of the first pass's ring"
        elif w == "two_turns":
            assert _crosses(first, length, LAG + N).any() and _crosses(first, length, 2 * N).any(), "no window across a ring's end on its second turn"
        else:
            raise ValueError(w)


# (content, H, W, D, usd, lsd, the windows the case is there for)
CASES = [
    # (no window holds the last row of the image: the first pass's ring, whose slot 0 takes row N, is crossed from N + 2 rows on)
    # heights, ragged width of 67: below the read-ahead of 16 rows, one past 16, below LAG + 1, around N, past two turns
    ("flat", 1, 67, 64, 34, 17, ["empty"]),
    ("flat", 2, 67, 64, 34, 17, ["short"]),
    ("noise", 2, 67, 64, 34, 17, ["short", "only_short"]),
    ("flat", 17, 67, 64, 34, 17, ["column"]),
    ("mondrian", 17, 67, 64, 34, 17, ["between"]),
    ("flat", 37, 67, 64, 34, 17, ["clipped"]),
    ("mondrian", 37, 67, 64, 34, 17, ["between"]),
    ("flat", N - 1, 67, 64, 34, 17, ["full", "wrap_in"]),
    ("mondrian", N - 1, 67, 64, 34, 17, ["between", "wrap_in"]),
    ("flat", N, 67, 64, 34, 17, ["full", "wrap_in"]),
    ("flat", N + 1, 67, 64, 34, 17, ["full", "wrap_in"]),
    ("mondrian", N + 1, 67, 64, 34, 17, ["between", "wrap_in"]),
    ("noise", N + 1, 67, 64, 34, 17, ["short", "only_short"]),
    ("synth", N + 1, 67, 64, 34, 17, ["wrap_in"]),
    ("flat", 2 * N + 5, 67, 64, 34, 17, ["full", "wrap_in", "wrap_mid", "two_turns"]),
    ("mondrian", 2 * N + 5, 67, 64, 34, 17, ["between", "wrap_in", "wrap_mid", "two_turns"]),
    # widths: one column, one group of four, one past a multiple of 64
    ("flat", N + 1, 1, 64, 34, 17, ["full", "wrap_in"]),
    ("mondrian", N + 1, 1, 64, 34, 17, ["wrap_in"]),
    ("flat", N + 1, 4, 64, 34, 17, ["full", "wrap_in"]),
    ("mondrian", N + 1, 4, 64, 34, 17, ["wrap_in"]),
    ("flat", 100, 129, 64, 34, 17, ["full", "full_count", "wrap_in", "wrap_mid"]),
    ("mondrian", 100, 129, 64, 34, 17, ["between", "wrap_in", "wrap_mid"]),
    ("synth", 100, 129, 64, 34, 17, ["wrap_in", "wrap_mid"]),
    ("noise", 100, 129, 64, 34, 17, ["short", "only_short"]),
    # a record with fifteen padding hypotheses
    ("flat", N + 1, 67, 49, 34, 17, ["full", "wrap_in"]),
    ("mondrian", 2 * N + 5, 67, 49, 34, 17, ["between", "wrap_in", "wrap_mid", "two_turns"]),
    ("mondrian", 37, 4, 49, 34, 17, ["between"]),
    # the arm limits: the shortest of the tests, and the longest the kernel takes (windows of N rows fill a ring)
    ("flat", 100, 129, 64, 29, 14, ["full", "full_count", "wrap_in", "wrap_mid"]),
    ("mondrian", 100, 129, 64, 29, 14, ["between", "wrap_in", "wrap_mid"]),
    ("flat", 100, 129, 64, 36, 18, ["full", "full_count", "wrap_in", "wrap_mid"]),
    ("mondrian", 100, 129, 64, 36, 18, ["between", "wrap_in", "wrap_mid"]),
    ("flat", 2 * N + 5, 67, 64, 36, 18, ["full", "wrap_in", "wrap_mid", "two_turns"]),
    ("mondrian", 2 * N + 5, 67, 64, 36, 18, ["between", "wrap_in", "wrap_mid", "two_turns"]),
    ("noise", N, 4, 64, 36, 18, ["short", "only_short"]),
    ("flat", N - 1, 1, 49, 36, 18, ["clipped", "wrap_in"]),
    ("flat", 1, 1, 64, 36, 18, ["empty"]),
    ("flat", 17, 129, 64, 29, 14, ["column"]),
    # columns that do not fill a round of the chip's wave slots are cut into row ranges of 128 rows and more, one wave each: two
    # ranges, and three of unequal length
    ("mondrian", 300, 67, 64, 34, 17, ["between", "wrap_in", "wrap_mid", "two_turns"]),
    ("flat", 300, 4, 64, 34, 17, ["full", "wrap_in", "wrap_mid", "two_turns"]),
    ("mondrian", 400, 4, 64, 36, 18, ["between", "wrap_in", "wrap_mid", "two_turns"]),
    ("flat", 400, 1, 49, 36, 18, ["full", "wrap_in", "wrap_mid", "two_turns"]),
]


@pytest.mark.parametrize("content, H, W, D, usd, lsd, wants", CASES, ids=["%s-%dx%d-D%d-usd%d" % c[:5] for c in CASES])
def test_v2_and_maps(gpu_ready, orc, content, H, W, D, usd, lsd, wants):
    p = tap._params(D=D, usd=usd, lsd=lsd)
    pair = _pair(content, H, W, p)
    _assert_holds(wants, tap._arms(orc, pair, p), usd, H, W)
    tap.assert_form(tap.DEFAULT, p, H, W)
    tap.assert_form(MFMA, p, H, W)
    ref = tap._chain(orc, pair, p)
    tag = "%s %dx%d D%d usd%d" % (content, H, W, D, usd)
    got = tap.run_tapped(pair, p, 1, 0)
    tap._same_volume(got["v2"], ref["v2"], tag + ", vector adds, after both vertical passes")
    assert got["maps"].tobytes() == ref["maps"].tobytes(), tag + ", vector adds, the WTA maps"
    mfma = tap.run_tapped(pair, p, 1, MFMA.variant)
    tap._same_volume(mfma["v2"], got["v2"], tag + ", the MFMA variant against the default")
    assert mfma["maps"].tobytes() == got["maps"].tobytes(), tag + ", the maps of the MFMA variant against the default's"


def test_refined_frame_under_both_variants(gpu_ready):
    """stages = 3 (matching and refinement) through stm_d_adcensus_stm: both maps and the output image, default against MFMA variant"""
    import torch
    import stm_amd
    from stm_amd import device_api as dev
    H, W = 100, 129
    p = tap._params()
    pair = tap._pair("synth", H, W, p)
    sbs = torch.from_numpy(tc.sbs_of(np.array(pair[0]), np.array(pair[1]))).cuda()
    outs = []
    for variant in (0, MFMA.variant):
        dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
        dr = torch.zeros_like(dl)
        out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
        stm_amd.lib().stm_set_agg_variant(variant)
        try:
            dev.d_adcensus_stm(sbs, dl, dr, out, p, stages=3)
            torch.cuda.synchronize()
        finally:
            stm_amd.lib().stm_set_agg_variant(0)
        outs.append((dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()))
    assert np.isfinite(outs[0][0]).all() and np.isfinite(outs[0][1]).all()
    for a, b, what in zip(outs[0], outs[1], ("left map", "right map", "output image")):
        assert a.tobytes() == b.tobytes(), what
