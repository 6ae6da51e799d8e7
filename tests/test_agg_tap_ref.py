"""The cases of tests/test_gpu_agg_tap.py judged on the CPU oracle alone: what makes them worth running on the GPU.

The frame's aggregation kernels are compared with the oracle through stm_set_agg_tap as volumes; the last horizontal pass, which is
fused with WTA, is compared through its maps on volumes injected in front of it.  Here: the content gives the arms every length; on
the planted volumes every single-element window fault, a padding guard one too strict and both wrong pixel-major orders change a
map; and -- the reason the tap exists -- on the suite's ordinary synthetic content the same kind of fault changes next to nothing."""
import numpy as np
import pytest

import agg_tap_cases as tc

SHAPES = [(64, 100, 129), (64, 37, 67), (64, 4, 300), (64, 2, 300), (49, 53, 67), (100, 37, 67)]


@pytest.mark.parametrize("H, W", [(100, 129), (37, 67), (53, 67)])
def test_mondrian_arms_take_every_length(orc, H, W):
    """both views: arms 0 (the border), lsd and usd occur along rows and along columns, and every length between along rows"""
    for v, img in enumerate(tc.mondrian_pair(H, W)):
        cross = orc.cross_arms(img, tc.UCD, tc.LCD, tc.USD, tc.LSD)
        for name, planes in (("vertical", cross[:2]), ("horizontal", cross[2:])):
            have = set(np.unique(planes).tolist())
            want = {0, tc.LSD, tc.USD}
            assert want <= have, "view %d, %s arms: %r missing" % (v, name, sorted(want - have))
        assert set(range(tc.USD + 1)) <= set(np.unique(cross[2:]).tolist()), "view %d: a horizontal arm length never occurs" % v
        assert int(cross.max()) == tc.USD


@pytest.mark.parametrize("H, W", [(2, 300), (2, 700), (17, 200)])
def test_mondrian_rows_of_the_flat_shapes(orc, H, W):
    """the shapes of a few rows: horizontal arms 0, lsd and usd in both views"""
    for v, img in enumerate(tc.mondrian_pair(H, W)):
        cross = orc.cross_arms(img, tc.UCD, tc.LCD, tc.USD, tc.LSD)
        assert {0, tc.LSD, tc.USD} <= set(np.unique(cross[2:]).tolist()), v


def test_planted_volumes_are_exact_and_cover_every_hypothesis():
    for D, H, W in SHAPES:
        planted = np.zeros((D, 2), bool)  # [d] planted in some row, unplanted in another
        for name, vol in tc.planted_volumes(D, H, W):
            assert vol.dtype == np.float32 and vol.shape == (D, H, W)
            low = vol < vol.max(axis=0, keepdims=True)  # [d][y][x]: lowered against the plane
            rows = low.all(axis=2)
            assert np.array_equal(rows, low.any(axis=2))
            assert (rows.sum(axis=0) == (0 if name == "ties" else 1)).all()
            planted[:, 0] |= rows.any(axis=1)
            planted[:, 1] |= (~rows).any(axis=1)
            # 2 * 255 elements of at most 4: the sums need 11 bits above the point and 10 below
            assert np.array_equal(vol * 1024, np.round(vol * 1024)) and vol.max() <= 4 and vol.min() >= 1 - tc.EPS
        assert planted.all(), (D, H, W)


def _maps_differ(orc, a, b, zd):
    return int(np.count_nonzero(orc.dc_wta(a, zd) != orc.dc_wta(b, zd)))


@pytest.mark.parametrize("D, H, W", SHAPES, ids=["D%d_%dx%d" % s for s in SHAPES])
def test_every_window_fault_changes_a_map(orc, D, H, W):
    """For every d < D, both residues and both signs: one window element dropped or counted twice at the columns x % 16 == r changes
    dc_wta in at least one pixel of at least one planted volume.  So do the last plane copied from its neighbour and, for D = 64, the
    two wrong hypothesis orders of a pixel-major record.  Zero misses."""
    zd = D // 2
    img = tc.mondrian_pair(H, W)[0]
    cross = orc.cross_arms(img, tc.UCD, tc.LCD, tc.USD, tc.LSD)
    vols = [(v, orc.agg_hpass(v, cross)) for _, v in tc.planted_volumes(D, H, W)]
    for src, agg in vols:
        assert np.array_equal(agg * 1024, np.round(agg * 1024))  # exact sums
    muts = tc.window_mutations(D) + tc.layout_mutations(D)
    assert len(muts) == 4 * D + (3 if D == 64 else 1)
    missed = [name for name, f in muts if not any(_maps_differ(orc, agg, f(agg, src), zd) for src, agg in vols)]
    assert not missed, "%d of %d mutations change no map: %r" % (len(missed), len(muts), missed[:8])


def test_planted_rows_have_the_planted_winner(orc):
    """in a row the planted hypothesis wins wherever the window is not empty, and hypothesis 0 where it is and in the volume of ties"""
    D, H, W, zd = 64, 37, 67, 20
    cross = orc.cross_arms(tc.mondrian_pair(H, W)[1], tc.UCD, tc.LCD, tc.USD, tc.LSD)
    empty = (cross[2].astype(int) + cross[3]) == 0
    for off, (name, vol) in zip(tc.plant_offsets(D, H) + [None], tc.planted_volumes(D, H, W)):
        got = orc.dc_wta(orc.agg_hpass(vol, cross), zd)
        want = np.zeros((H, W)) if off is None else np.where(empty, 0, ((np.arange(H) + off) % D)[:, None])
        assert np.array_equal(got, (want - zd).astype(np.float32)), name


def test_noise_volume():
    v = tc.noise_volume(64, 37, 67)
    assert v.dtype == np.float32 and v.min() >= 1.0 and v.max() < 2.0 and len(np.unique(v)) > v.size // 2


def test_setter_refuses_a_misaligned_buffer_and_keeps_the_tap(stm):
    """stm_set_agg_tap in the style of the other setters: -1 with stm_last_error under error mode 1, 0 for pointers it can take and
    for all four null (host logic only: nothing is launched, no device is touched)"""
    lib = stm.lib()
    lib.stm_set_error_mode(1)
    try:
        for k, name in enumerate((b"d_h1", b"d_v2", b"d_h4", b"d_inject_v2")):
            args = [None] * 4
            args[k] = 0x1002
            assert lib.stm_set_agg_tap(*args) == -1
            assert b"set_agg_tap" in lib.stm_last_error() and name in lib.stm_last_error()
        assert lib.stm_set_agg_tap(None, None, None, None) == 0
    finally:
        lib.stm_set_agg_tap(None, None, None, None)
        lib.stm_set_error_mode(0)


def test_argmin_on_ordinary_content_sees_next_to_nothing(orc):
    """The weakness the tap answers, stated once: on synth.sbs_frame at 100 x 129 (D 64, usd 34 / lsd 17) a first pass that drops a
    window element at every sixteenth column of every hypothesis, three hypotheses 2 % high at every 96th column after the first
    pass, and four hypotheses 1 % high at every 64th column of the final volume each change at most 1 % of the WTA pixels of either
    view.  If this fails the synthetic content has become sharp enough for the maps to notice, and the statement needs revisiting."""
    from stm_amd import synth
    D, zd, H, W = 64, 32, 100, 129
    sbs = synth.sbs_frame(H, W, D, zd)[0]
    L, R = np.ascontiguousarray(sbs[:, :W]), np.ascontiguousarray(sbs[:, W:])
    costs = orc.ci_adcensus(L, R, 10.0, 30.0, D, zd)
    for v, img in enumerate((L, R)):
        cross = orc.cross_arms(img, tc.UCD, tc.LCD, tc.USD, tc.LSD)
        h1 = orc.agg_hpass(costs[v], cross)
        rest = lambda vol: orc.agg_hpass(orc.agg_vpass(orc.agg_vpass(vol, cross), cross), cross)
        final = rest(h1)
        for name, f in tc.argmin_blind_mutations():
            h1m, fm = f(costs[v], cross, h1, final)
            mutated = rest(h1m) if h1m is not None else fm
            assert int(np.count_nonzero(mutated != final)) >= 4 * H * (W // 64), name  # the fault is there, in hundreds of costs
            changed = _maps_differ(orc, final, mutated, zd)
            assert changed <= H * W // 100, "view %d, %s: %d WTA pixels changed" % (v, name, changed)
