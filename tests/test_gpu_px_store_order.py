"""The hypothesis order inside a pixel's record of the pixel-major (PX) volumes (stm_px_order).

By default the first pass (stm_k_pq_hc2, stm_k_pq_hc<8 / 12, true>) writes hypothesis 16 b + n of a pixel at float 4 n + b of its
256-byte record, which is what lets a lane store its four accumulator registers b = 0 .. 3 as 16 bytes; the second pass of
stm_k_pq_v12r does the same to the floats it holds, and stm_k_pq_hsr's WTA and its d >= D guard take the hypothesis a lane
carries -- 4 n + b for chunk b of lane n after both -- from the order.  stm_set_agg_variant(2000000000) keeps the ascending order
and the 4-byte stores in both kernels.  The maps cannot depend on the order, so every
case runs stm_d_adcensus_stm at stages 1 and 3 under both, compares each with the CPU oracle element for element (disp_l, disp_r,
interlaced) and the two with each other, after asking the dispatcher (stm_agg_path, stm_first_pass_path, stm_px_order) that the
form the case names is the one that runs.

What a wrong lane <-> hypothesis map gets wrong: which lanes are padding (d >= D) when D < 64 -- 49 and 63 leave a partly filled
chunk and a partly filled lane quad --, and which of several hypotheses at the minimum wins (the lowest true d), which random
content rarely asks.  The tie cases first check on the oracle's own aggregated volume that they are tie cases."""
import numpy as np
import pytest

from test_gpu_px_layout import _oracle, _run

pytestmark = pytest.mark.gpu

ORDER_0 = 2000000000  # ascending hypotheses, sixteen 4-byte stores per tile
DEFAULT_ORDER = 2  # stm_px_order: the permutation of a 16-byte store applied twice, by the first pass and by stm_k_pq_v12r
SEPARATE_VIEWS = 2000000  # stm_k_pq_hc<12, true> where the default runs stm_k_pq_hc2
HC2, HC8, HC12 = "stm_k_pq_hc2", "stm_k_pq_hc<8, true>", "stm_k_pq_hc<12, true>"

_want = {}  # oracle results, computed once per input and shared by the cases that use it


def _p(D, zd, usd=34, lsd=17):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd)


def _content(H, W, p):
    from stm_amd import synth
    return synth.sbs_frame(H, W, p.num_disp, min(max(p.zero_disp, 0), p.num_disp - 1))[0]


def _sbs(L, R):
    return np.ascontiguousarray(np.concatenate([L, R], axis=1))


def _forms(p, H, W, variant):
    """(agg_path, first_pass_path, px_order) of stages 1 and 3 under `variant`; both stages agree"""
    import stm_amd
    from stm_amd import device_api as dev
    a = (p.num_disp, p.zero_disp, H, W, p.usd)
    stm_amd.lib().stm_set_agg_variant(variant)
    try:
        got = [(dev.agg_path(*a, s), dev.first_pass_path(*a, s), dev.px_order(*a, s)) for s in (1, 3)]
    finally:
        stm_amd.lib().stm_set_agg_variant(0)
    assert got[0] == got[1], got
    return got[0]


def _assert_form(p, H, W, kernel, parts=None, base=0):
    """The dispatcher runs `kernel` as the first pass of this case on PX volumes, in the default order under variant `base` and in order 0
    under base + ORDER_0, and nothing else differs between the two."""
    from stm_amd import device_api as dev
    path, fp, order = _forms(p, H, W, base)
    assert path & dev.AGG_PX and path & dev.AGG_VREGS and path & dev.AGG_HREGS, hex(path)
    assert order == DEFAULT_ORDER, order
    if kernel == HC2:
        assert fp >= 1 and dev.agg_path_waves(path) == 12, (fp, hex(path))
        assert parts is None or fp == parts, fp
    else:
        assert fp == 0 and dev.agg_path_waves(path) == (8 if kernel == HC8 else 12), (fp, hex(path))
    assert _forms(p, H, W, base + ORDER_0) == (path, fp, 0)


def _check(orc, key, sbs, p, H, W, kernel, parts=None, base=0):
    assert sbs.shape == (H, 2 * W, 3) and sbs.dtype == np.uint8
    _assert_form(p, H, W, kernel, parts, base)
    if key not in _want:
        _want[key] = _oracle(orc, sbs, p, H, W)
    want = _want[key]
    got = {}
    for variant in (base, base + ORDER_0):
        w_l, w_r, _ = _run(sbs, p, 1, H, W, variant)
        assert np.array_equal(w_l, want["wta_l"].astype(np.float32)), "wta_l, variant %d" % variant
        assert np.array_equal(w_r, want["wta_r"].astype(np.float32)), "wta_r, variant %d" % variant
        dl, dr, out = _run(sbs, p, 3, H, W, variant)
        assert np.array_equal(dl, want["disp_l"]), "disp_l, variant %d" % variant
        assert np.array_equal(dr, want["disp_r"]), "disp_r, variant %d" % variant
        assert np.array_equal(out, want["interlaced"]), "interlaced, variant %d" % variant
        got[variant] = (w_l, w_r, dl, dr, out)
    for a, b in zip(got[base], got[base + ORDER_0]):
        assert np.array_equal(a, b), "the default order against order 0"


ZD = [(32, HC2), (0, HC8)]  # inside 18..45 the 12-wave form, which is stm_k_pq_hc2's; outside it stm_k_pq_hc<8, true> (usd 34)


@pytest.mark.parametrize("zd, kernel", ZD, ids=["zd32_hc2", "zd0_hc8"])
@pytest.mark.parametrize("shape", [(33, 80), (50, 97)], ids=["80x33", "97x50"])
@pytest.mark.parametrize("D", [49, 56, 63, 64])
def test_padded_hypotheses_and_ragged_frames(gpu_ready, orc, D, shape, zd, kernel):
    """D = 49 and 63: a partly filled chunk of 16 and a partly filled quad of four lanes; 56: the two last lanes of a quad-row are padding
    in every chunk by default (hypotheses 4 n + b >= 56 are lanes n = 14, 15), half the last chunk in order 0.  80 x 33 and 97 x 50: H = 16 k + 1
    and 16 k + 2, W = 97 not a multiple of 4, so the last tile's and the last row's 16-byte stores end where the allocation
    ends and the buffer's range check is what drops the rest."""
    H, W = shape
    p = _p(D, zd)
    _check(orc, ("content", D, H, W, zd), _content(H, W, p), p, H, W, kernel)


@pytest.mark.parametrize("base, kernel", [(SEPARATE_VIEWS, HC12)], ids=["hc12"])
@pytest.mark.parametrize("D", [49, 64])
def test_one_view_per_block_form(gpu_ready, orc, D, base, kernel):
    """stm_k_pq_hc<12, true> runs only under variant 2000000; it has both store forms too.  97 x 50, zero_disp 32."""
    H, W = 50, 97
    p = _p(D, 32)
    _check(orc, ("content", D, H, W, 32), _content(H, W, p), p, H, W, kernel, base=base)


def _stripes(H, W, period):
    """vertical stripes: column x has grey level 60 + 40 ((x mod period) >= period / 2), the same in both eyes"""
    col = (60 + 40 * ((np.arange(W) % period) >= period // 2)).astype(np.uint8)
    return np.repeat(np.repeat(col[None, :, None], H, axis=0), 3, axis=2)


def _tie_share(orc, L, R, p):
    """share of the pixels of either view at which more than one hypothesis holds the minimum of the oracle's aggregated volume"""
    cl, cr = orc.ci_adcensus(L, R, p.ad_coeff, p.census_coeff, p.num_disp, p.zero_disp)
    shares = []
    for img, cost in ((L, cl), (R, cr)):
        _, acost = orc.ca_cross(img, cost, p.ucd, p.lcd, p.usd, p.lsd)
        shares.append(float(((acost == acost.min(axis=0)[None]).sum(axis=0) > 1).mean()))
    return min(shares)


TIES = ["flat", "stripes4", "stripes16"]


@pytest.mark.parametrize("zd, kernel", ZD, ids=["zd32_hc2", "zd0_hc8"])
@pytest.mark.parametrize("D", [64, 49])
@pytest.mark.parametrize("pattern", TIES)
def test_ties_go_to_the_lowest_hypothesis(gpu_ready, orc, pattern, D, zd, kernel):
    """97 x 50, both eyes the same image: one colour, or vertical stripes of period 4 and 16.  Shifting by a multiple of the period
    (by anything, for the flat pair) gives the same costs, so many hypotheses tie exactly at the minimum and WTA must return the
    lowest true d -- where the lane <-> hypothesis map of the last pass decides the result.  The share of such pixels is checked
    on the oracle's aggregated volume first: at least a quarter of either view."""
    H, W = 50, 97
    img = np.full((H, W, 3), 93, np.uint8) if pattern == "flat" else _stripes(H, W, 4 if pattern == "stripes4" else 16)
    p = _p(D, zd)
    key = ("ties", pattern, D, zd)
    if key not in _want:
        share = _tie_share(orc, img, img, p)
        print("ties, %s, D %d, zd %d: %.3f of the pixels" % (pattern, D, zd, share))
        assert share >= 0.25, share
    _check(orc, key, _sbs(img, img), p, H, W, kernel)


@pytest.mark.parametrize("zd, usd, kernel", [(32, 36, HC2), (0, 36, HC8), (32, 5, HC2), (0, 5, HC2)],
                         ids=["usd36_hc2", "usd36_hc8", "usd5_zd32", "usd5_zd0"])
def test_longest_and_shortest_sweeps(gpu_ready, orc, zd, usd, kernel):
    """64 x 48, D = 64: usd 36, the longest sweep of all three kernels (with the halo of usd 36 zero_disp 0 takes the 8-wave
    form), and usd 5, the shortest halo (HG = 4), where the 12-wave form and with it stm_k_pq_hc2 holds for every zero_disp."""
    H, W = 48, 64
    p = _p(64, zd, usd, (usd + 1) // 2)
    _check(orc, ("content", 64, H, W, zd, usd), _content(H, W, p), p, H, W, kernel)


def _smallest_two_part_frame():
    """the smallest H, then W, at which stm_k_pq_hc2 splits a row (host query; D 64, zero_disp 32, usd 34)"""
    from stm_amd import device_api as dev
    for H in range(1, 4):
        for W in range(1, 1200):
            if dev.first_pass_path(64, 32, H, W, 34, 3) == 2:
                return H, W
    raise AssertionError("no frame below 4 x 1200 with two parts per row")


def test_row_parts(gpu_ready, orc):
    """A row in two parts of stm_k_pq_hc2 (each fills its own ring and stores its own tiles) and several of stm_k_pq_hsr: the
    smallest such frame, one row of 673 pixels = eight segments of 96, and the same width at 17 rows."""
    H, W = _smallest_two_part_frame()
    assert (H, W) == (1, 673)
    for H in (1, 17):
        p = _p(64, 32)
        _check(orc, ("content", 64, H, W, 32), _content(H, W, p), p, H, W, HC2, parts=2)
