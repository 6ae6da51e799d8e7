"""The pixel-major (PX) fast path of the frame at both forms of its first pass and at the edges of all three kernels:
stm_k_pq_hc<12, true> and stm_k_pq_hc<8, true> (which hc_waves picks from zero_disp and the halo of usd), their row split, the
staging limit, padded last chunks with the match range at one end, frames smaller than a tile or a segment, arms at their limits,
whole volumes of ties, and the matching parameters.

Every case first asks stm_agg_path which form the dispatcher takes and asserts that it is the one the case names, so a retune of
hc_waves' budget fails here (and in tests/test_agg_path.py) instead of moving the cases onto another kernel.  Every comparison is
element for element with the CPU oracle, for the default build and for stm_set_agg_variant(20000000), the PQ layout end to end."""
import numpy as np
import pytest

from conftest import rand_pair
from test_gpu_parity import _fuzz_cases
from test_gpu_px_layout import PQ_END_TO_END, _oracle, _run

pytestmark = pytest.mark.gpu

NOT_PX = 0  # as a case's form: the chain keeps the PQ layout


def _p(D, zd, usd=34, lsd=17, **kw):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=zd, usd=usd, lsd=lsd, **kw)


def _content(H, W, p, seed=None):
    """synth.sbs_frame content; its ground truth is laid out for a zero_disp inside [0, D)"""
    from stm_amd import synth
    zd = min(max(p.zero_disp, 0), p.num_disp - 1)
    return synth.sbs_frame(H, W, p.num_disp, zd)[0] if seed is None else synth.sbs_frame(H, W, p.num_disp, zd, seed=seed)[0]


def _assert_form(p, H, W, stages, form, split):
    """the default build on PX with `form` waves in stm_k_pq_hc (NOT_PX: off it), its row split or not; 20000000 never on PX"""
    import stm_amd
    from stm_amd import device_api as dev
    lib = stm_amd.lib()
    got = dev.agg_path(p.num_disp, p.zero_disp, H, W, p.usd, stages)
    assert got & dev.AGG_MATRIX_PIPE, hex(got)
    assert bool(got & dev.AGG_PX) == (form != NOT_PX), "PX, path 0x%x" % got
    if form != NOT_PX:
        assert dev.agg_path_waves(got) == form, "waves, path 0x%x" % got
        assert got & dev.AGG_VREGS and got & dev.AGG_HREGS, hex(got)
    assert bool(got & dev.AGG_SPLIT) == split, "row split, path 0x%x" % got
    lib.stm_set_agg_variant(PQ_END_TO_END)
    try:
        pq = dev.agg_path(p.num_disp, p.zero_disp, H, W, p.usd, stages)
    finally:
        lib.stm_set_agg_variant(0)
    assert pq & dev.AGG_MATRIX_PIPE and not pq & dev.AGG_PX, hex(pq)
    return got


def _check(orc, sbs, p, H, W, form, split=False, wta_only=False):
    """The case is on the form it names; then stages = 1 (raw WTA maps) and stages = 3 (maps and interlaced frame) of the default
    build and of the PQ variant against the oracle, element for element.  wta_only: stages = 1 alone, against the oracle stopped
    after WTA."""
    assert sbs.shape == (H, 2 * W, 3) and sbs.dtype == np.uint8
    got = _assert_form(p, H, W, 1, form, split)
    assert _assert_form(p, H, W, 3, form, split) == got
    if wta_only:
        want = orc.adcensus_stm(sbs, H, W, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd,
                                p.usd, p.lsd, p.thresh_s, p.thresh_h, stop_after_wta=True)
    else:
        want = _oracle(orc, sbs, p, H, W)
    for variant in (0, PQ_END_TO_END):
        w_l, w_r, _ = _run(sbs, p, 1, H, W, variant)
        assert np.array_equal(w_l, want["wta_l"].astype(np.float32)), "wta_l, variant %d" % variant
        assert np.array_equal(w_r, want["wta_r"].astype(np.float32)), "wta_r, variant %d" % variant
        if wta_only:
            continue
        dl, dr, out = _run(sbs, p, 3, H, W, variant)
        assert np.array_equal(dl, want["disp_l"]) and np.array_equal(dr, want["disp_r"]), "disparities, variant %d" % variant
        assert np.array_equal(out, want["interlaced"]), "interlaced, variant %d" % variant
    return got


# zero_disp -> the form at D = 64 with the halo of usd 29..36: pad = max(zd, 63 - zd) + 15 <= 60 fits the 12-wave block's LDS budget
ZD_FORMS = [(0, 8), (17, 8), (18, 12), (45, 12), (46, 8), (63, 8), (-3, 8), (67, 8)]


@pytest.mark.parametrize("zd, form", ZD_FORMS, ids=["zd%d" % z for z, _ in ZD_FORMS])
@pytest.mark.parametrize("shape", [(37, 67), (100, 129), (100, 257)], ids=["37x67", "100x129", "100x257"])
def test_first_pass_forms_over_zero_disp(gpu_ready, orc, shape, zd, form):
    """D = 64, usd 34 / lsd 17.  zd 0 (parallel cameras), 17, 46, 63 and the two outside [0, D): stm_k_pq_hc<8, true>, its PX
    stores, its 128-pixel segments and its 128 + 2 pad staging; 18 and 45: the last values on stm_k_pq_hc<12, true>.  37 x 67: less
    than one segment of either; 100 x 129 and 100 x 257: one pixel past one and past two 128-pixel segments."""
    H, W = shape
    p = _p(64, zd)
    _check(orc, _content(H, W, p), p, H, W, form)


@pytest.mark.parametrize("zd, form", [(177, 8), (178, NOT_PX)])
def test_staging_limit(gpu_ready, orc, zd, form):
    """D = 64, usd 34, 24 x 150, raw WTA maps.  zd 177: pad = 192, SO = 128 + 2 pad = 512 staged pixels, one for every thread of the
    8-wave block; zd 178: the first value that leaves stm_k_pq_hc and with it the PX layout.  (No hypothesis has a partner inside
    the frame; the costs are the border rule's.)"""
    H, W = 24, 150
    p = _p(64, zd)
    _check(orc, _content(H, W, p), p, H, W, form, wta_only=True)


@pytest.mark.parametrize("D, usd, lsd", [(48, 34, 17), (65, 34, 17), (64, 37, 18)], ids=["D48", "D65", "usd37"])
def test_first_values_off_px(gpu_ready, orc, D, usd, lsd):
    """The neighbours of the PX range on either side of num_disp and past usd 36, 53 x 67 at zero_disp D // 2: stm_agg_path reports
    the PQ layout (three and five chunks; the LDS-ring vertical kernel) and the frame is the oracle's all the same."""
    H, W = 53, 67
    p = _p(D, D // 2, usd, lsd)
    _check(orc, _content(H, W, p), p, H, W, NOT_PX)


@pytest.mark.parametrize("usd, lsd", [(34, 17), (28, 14)], ids=["usd34", "usd28"])
@pytest.mark.parametrize("end", ["zd0", "zdD-1"])
@pytest.mark.parametrize("D", [49, 56, 57, 63])
def test_padded_last_chunk_with_the_range_at_one_end(gpu_ready, orc, D, end, usd, lsd):
    """49 <= D < 64: hypotheses D .. 63 of a PX pixel are padding that must never win, also where every real hypothesis reaches
    outside the frame; zero_disp 0 and D - 1 put the whole match range on one side.  pad = D - 1 + 15 > 60: the 8-wave form with
    the halo of usd 34, the 12-wave form with the shorter halo of usd 28."""
    H, W = 37, 67
    p = _p(D, 0 if end == "zd0" else D - 1, usd, lsd)
    _check(orc, _content(H, W, p), p, H, W, 8 if usd == 34 else 12)


@pytest.mark.parametrize("usd, form", [(4, 12), (5, 12), (28, 12), (29, 8)])
def test_halo_steps(gpu_ready, orc, usd, form):
    """D = 64, zd 0, 70 x 40.  The halo of the first pass is HG = 2, 4, 8 and 10 groups for usd 4, 5, 28 and 29; only the last
    pushes the 12-wave block past its LDS budget at pad = 78."""
    H, W = 70, 40
    p = _p(64, 0, usd, (usd + 1) // 2)
    _check(orc, _content(H, W, p), p, H, W, form)


@pytest.mark.parametrize("W, zd, form", [(3100, 0, 8), (4700, 32, 12)], ids=["3100_8waves", "4700_12waves"])
def test_row_split(gpu_ready, orc, W, zd, form):
    """Three rows, D = 64, more than 24 segments each: a row of stm_k_pq_hc is split over two blocks (3100 > 24 * 128 with the
    8-wave form, 4700 > 24 * 192 with the 12-wave form), each of which fills its own ring from the middle of the row."""
    H = 3
    p = _p(64, zd)
    _check(orc, _content(H, W, p), p, H, W, form, split=True)


SMALL = [(1, 1), (1, 2), (2, 3), (1, 70), (70, 1), (15, 5), (17, 4), (200, 5)]


@pytest.mark.parametrize("zd, form", [(0, 8), (32, 12)], ids=["zd0", "zd32"])
@pytest.mark.parametrize("shape", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_few_rows_or_columns(gpu_ready, orc, shape, zd, form):
    """D = 64, usd 36 / lsd 18: fewer than 9 rows, fewer than 13 columns, one pixel, one row, one column, one row more than a
    tile, one group of four columns, and 200 rows of five columns (every sweep at the full length of the arms)."""
    H, W = shape
    p = _p(64, zd, 36, 18)
    _check(orc, _content(H, W, p), p, H, W, form)


def _sbs(L, R):
    return np.ascontiguousarray(np.concatenate([L, R], axis=1))


@pytest.mark.parametrize("zd_of", ["zd0", "zdmid"])
@pytest.mark.parametrize("D", [64, 50])
def test_flat_pair_is_a_volume_of_ties(gpu_ready, orc, D, zd_of):
    """120 x 40, usd 36 / lsd 36, both eyes one colour: every arm is 36 long or stops at the border, and every hypothesis of a pixel
    has the same aggregated cost wherever its partner is inside the frame, so WTA resolves a whole volume of ties -- as the oracle
    does.  D = 50: the padded hypotheses 50 .. 63 hold zeros that tie with, or undercut, the real ones and still must not win."""
    H, W = 120, 40
    zd = 0 if zd_of == "zd0" else D // 2
    flat = np.full((H, W, 3), 93, np.uint8)
    p = _p(D, zd, 36, 36)
    _check(orc, _sbs(flat, flat), p, H, W, 8 if zd == 0 else 12)


@pytest.mark.parametrize("zd, form", [(0, 8), (32, 12)], ids=["zd0", "zd32"])
def test_ramp_in_one_eye(gpu_ready, orc, zd, form):
    """120 x 40, D = 64, usd 36 / lsd 36: the left eye a horizontal ramp of two grey levels per column, the right eye flat.  The
    right view's arms are at the limits, the left view's horizontal arms are cut by the colour rule, and the costs tie in runs."""
    H, W = 120, 40
    ramp = np.repeat((np.arange(W, dtype=np.int32) * 2 + 60)[None, :, None], H, axis=0).repeat(3, axis=2).astype(np.uint8)
    flat = np.full((H, W, 3), 100, np.uint8)
    p = _p(64, zd, 36, 36)
    _check(orc, _sbs(ramp, flat), p, H, W, form)


@pytest.mark.parametrize("zd, form", [(0, 8), (32, 12)], ids=["zd0", "zd32"])
def test_shortest_arms(gpu_ready, orc, zd, form):
    """120 x 40, D = 64, usd 36 / lsd 36, ucd = lcd = 0 on blocks of noise-free colour: an arm runs only over pixels of exactly the
    anchor's colour"""
    H, W = 120, 40
    L, R = rand_pair(H, W, 77, smooth=False)
    p = _p(64, zd, 36, 36, ucd=0.0, lcd=0.0)
    _check(orc, _sbs(L, R), p, H, W, form)


@pytest.mark.parametrize("zd, form", [(0, 8), (32, 12)], ids=["zd0", "zd32"])
def test_longest_arms_on_content(gpu_ready, orc, zd, form):
    """120 x 40, D = 64, usd 36 / lsd 36, ucd = 60, lcd = 255 on synthetic content: the colour rule stops almost no arm"""
    H, W = 120, 40
    p = _p(64, zd, 36, 36, ucd=60.0, lcd=255.0)
    _check(orc, _content(H, W, p), p, H, W, form)


# the sweep of test_gpu_parity.py::test_random_frames_and_parameters -- the same draws from the same lists -- moved onto the PX
# chain: D in 49..64, usd in 1..36, zero_disp in [0, D) (15 %: outside by up to 3), H in 1..90, W in 2..300.  Seed chosen with
# stm_agg_path, on a machine without a GPU, so that both forms get at least five of the twenty cases (this one: five on the 8-wave form,
# which needs usd >= 29 and zero_disp outside [18, 45], and fifteen on the 12-wave form).
PX_FUZZ = _fuzz_cases(20, 20261119, H=(1, 90), W=(2, 301), D=(49, 65), usd=(1, 37))


def _fuzz_params(c):
    return _p(c["D"], c["zd"], c["usd"], c["lsd"], num_views=c["views"], angle=c["angle"], ad_coeff=c["ad"], census_coeff=c["cen"],
              ucd=c["ucd"], lcd=c["lcd"], thresh_s=c["ts"], thresh_h=c["th"])


def _fuzz_forms():
    from stm_amd import device_api as dev
    return [dev.agg_path_waves(dev.agg_path(c["D"], c["zd"], c["H"], c["W"], c["usd"], 3)) for c in PX_FUZZ]


def test_parameter_sweep_covers_both_forms(gpu_ready):
    forms = _fuzz_forms()
    assert len(forms) == 20 and set(forms) <= {8, 12}, forms
    assert forms.count(8) >= 5 and forms.count(12) >= 5, forms


@pytest.mark.parametrize("i", range(20), ids=["%02d_%dx%d_D%d_zd%d_usd%d" % (i, c["H"], c["W"], c["D"], c["zd"], c["usd"])
                                              for i, c in enumerate(PX_FUZZ)])
def test_matching_parameters_on_px(gpu_ready, orc, i):
    """ad_coeff, census_coeff, ucd, lcd, the voting thresholds, 2..9 views, the angle and pure-noise pairs on the PX chain, in
    whichever form the draw lands on"""
    c = PX_FUZZ[i]
    H, W = c["H"], c["W"]
    p = _fuzz_params(c)
    if c["noise"]:
        L, R = rand_pair(max(H, 8), max(W, 8), c["seed"])
        sbs = _sbs(L[:H, :W], R[:H, :W])
    else:
        sbs = _content(H, W, p, seed=c["seed"])
    _check(orc, sbs, p, H, W, _fuzz_forms()[i])
