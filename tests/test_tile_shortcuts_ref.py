"""The conditions under which the cases of tests/tile_cases.py test what they are meant to test, asserted on the CPU oracle alone
(the GPU comparisons are in test_gpu_tile_shortcuts.py).  No GPU.

A case with one different pixel (or line) INSIDE the middle block's needed neighbourhood is worth something only if the expected
output of that block differs from the unperturbed map's: then a one-value shortcut taken by mistake shows.  A case with the pixel
OUTSIDE must leave the block's expected output as it was: there the shortcut is legitimate, and a kernel that takes it is right.
The gaussian kernel's shortcut rests on the filter returning a uniform map of 0 or 1 unchanged; the table test of the frame rests
on every value of the table filling the scanned region of at least one block of the map that enters the bilateral filter."""
import numpy as np
import pytest

import tile_cases as tc


def test_geometry_restated():
    """the numbers of the kernels (SF_TX = 16 threads x 4 pixels, SF_TY = 16, TW = (64 + 2R + 3) / 4 * 4 + 4)"""
    assert (tc.tile_width(7), tc.tile_width(10)) == (84, 88)
    assert tc.tile_width(7) - (tc.BW + 14) == 6 and tc.tile_width(10) - (tc.BW + 20) == 4
    assert tc.blocks(tc.STD_H, tc.STD_W) == [(y, x) for y in (0, 16, 32) for x in (0, 64, 128)]
    for R in (7, 10):  # the middle block's halo is not clamped, its padding columns are inside the map
        ys, xs = tc.scanned(tc.STD_H, tc.STD_W, R, tc.Y0, tc.X0)
        assert len(set(ys)) == tc.BH + 2 * R and len(set(xs)) == tc.tile_width(R)
        nys, nxs = tc.needed(tc.STD_H, tc.STD_W, R, tc.Y0, tc.X0)
        assert (nys[0], nys[-1], nxs[0], nxs[-1]) == (tc.Y0 - R, tc.Y0 + 15 + R, tc.X0 - R, tc.X0 + 63 + R)
    ys, xs = tc.scanned(15, 63, 7, 0, 0)
    assert ys.min() == 0 and ys.max() == 14 and xs.max() == 62
    m = tc.uniform(tc.STD_H, tc.STD_W, 3.0)
    assert len(tc.one_value_blocks(m, 7)) == 9
    m[tc.Y0 + 5, tc.X0 + 63 + 7 + 6] = 4.0  # the last padding column of the middle block at R = 7: scanned, not needed
    assert (tc.Y0, tc.X0, 3.0) not in tc.one_value_blocks(m, 7) and not tc.in_needed(7, tc.Y0 + 5, tc.X0 + 63 + 7 + 6)
    m = tc.uniform(tc.STD_H, tc.STD_W, 3.0)
    m[tc.Y0 + 5, tc.X0 + 63 + 7 + 7] = 4.0  # one further: not even scanned
    assert (tc.Y0, tc.X0, 3.0) in tc.one_value_blocks(m, 7)


@pytest.mark.parametrize("R", [10, 7, 3])
def test_sweep_covers_both_sides_of_every_edge(R):
    pos = tc.band_positions(R)
    inside = [p for p in pos if tc.in_needed(R, *p)]
    assert len(inside) >= 17 and len(pos) - len(inside) >= 17
    for y, x in [(tc.Y0 + 5, tc.X0 - R), (tc.Y0 + 5, tc.X0 + 63 + R), (tc.Y0 - R, tc.X0 + 9), (tc.Y0 + 15 + R, tc.X0 + 9),
                 (tc.Y0 - R, tc.X0 - R), (tc.Y0 + 15 + R, tc.X0 + 63 + R)]:
        assert (y, x) in inside
    for y, x in [(tc.Y0 + 5, tc.X0 - R - 1), (tc.Y0 + 5, tc.X0 + 64 + R), (tc.Y0 - R - 1, tc.X0 + 9), (tc.Y0 + 16 + R, tc.X0 + 9)]:
        assert (y, x) in pos and (y, x) not in inside


def _check_condition(name, inside, got, plain):
    """got / plain: the oracle's output for the case and for its unperturbed map"""
    if inside is True:
        assert not np.array_equal(tc.block_of(got), tc.block_of(plain)), name
    elif inside is False:
        assert np.array_equal(tc.block_of(got), tc.block_of(plain)), name


@pytest.mark.parametrize("R,sigma", tc.GAUSS_FAST + [tc.GAUSS_GENERIC])
def test_gaussian_cases_show_a_wrong_shortcut(orc, R, sigma):
    for b in (0.0, 1.0):
        for H, W in [(tc.STD_H, tc.STD_W)] + tc.EDGE_SHAPES:
            m = tc.uniform(H, W, b)
            assert np.array_equal(orc.filter_gaussian_1(m, R, sigma), m), (b, H, W)  # what the kernel's shortcut rests on
    seen = {True: 0, False: 0}
    for base, pixel in tc.GAUSS_PERTURB:
        plain = orc.filter_gaussian_1(tc.uniform(tc.STD_H, tc.STD_W, base), R, sigma)
        for name, m, inside in tc.pixel_sweep(R, base, pixel):
            _check_condition(name, inside, orc.filter_gaussian_1(m, R, sigma), plain)
            seen[inside] += 1
    assert seen[True] >= 34 and seen[False] >= 34
    # a lowered pixel changes nothing around it (grow-only): it would test nothing
    m = tc.uniform(tc.STD_H, tc.STD_W, 1.0)
    m[tc.Y0 - R, tc.X0 - R] = 0.0
    got = orc.filter_gaussian_1(m, R, sigma)
    assert np.array_equal(tc.block_of(got), tc.block_of(m))
    # the corner pixel reaches exactly one pixel of the block
    m = tc.uniform(tc.STD_H, tc.STD_W, 0.0)
    m[tc.Y0 - R, tc.X0 - R] = 1.0
    assert np.count_nonzero(tc.block_of(orc.filter_gaussian_1(m, R, sigma))) == 1
    # the mixed map has blocks of all three kinds
    assert tc.one_value_blocks(tc.gauss_mixed(R), R) == [(0, 0, 0.0), (tc.STD_H - tc.BH, tc.STD_W - tc.BW, 1.0)]
    assert tc.one_value_blocks(tc.gauss_thirds(), R) == []


@pytest.mark.parametrize("R,sigma", [(7, 10.0), (10, 15.0)], ids=["host_7", "device_10"])
def test_dbm_cases_show_a_wrong_shortcut(orc, R, sigma):
    il, ir, dl, dr, ml = tc.dbm_inputs()
    plain, seen = {}, {True: 0, False: 0}
    for name, mr, inside in tc.dbm_cases(R):
        got = orc.dibr_dbm(il, ir, dl, dr, ml, mr, tc.DBM_SHIFT, R, sigma)
        if inside is None:
            plain[float(mr[0, 0])] = got
            assert len(np.unique(got)) == 1, name
            continue
        _check_condition(name, inside, got, plain[float(mr[0, 0])])
        seen[inside] += 1
    assert seen == {True: 8, False: 8}
    # mask_l = 0: the blend never reaches the output, such a case would test nothing
    mr = tc.uniform(tc.STD_H, tc.STD_W, 1.0)
    mr[tc.Y0 - R, tc.X0:tc.X0 + tc.BW] = 0.0
    zero = np.zeros_like(ml)
    assert np.array_equal(orc.dibr_dbm(il, ir, dl, dr, zero, mr, tc.DBM_SHIFT, R, sigma),
                          orc.dibr_dbm(il, ir, dl, dr, zero, tc.uniform(tc.STD_H, tc.STD_W, 1.0), tc.DBM_SHIFT, R, sigma))


def test_bilateral_cases_show_a_wrong_form(orc):
    R, sc, ss = tc.BIL
    f = lambda m: orc.filter_bilateral_1(m, R, sc, ss, tc.BIL_D)
    seen = {True: 0, False: 0}
    for c in tc.BIL_SWEEP_BASES:
        plain = f(tc.uniform(tc.STD_H, tc.STD_W, c))
        assert len(np.unique(plain)) == 1  # one number for every pixel: what the one-value form stores
        for pixel in (c + 1.0, c + 0.5):
            for name, m, inside in tc.pixel_sweep(R, c, pixel):
                _check_condition(name, inside, f(m), plain)
                seen[inside] += 1
    assert seen[True] >= 68 and seen[False] >= 68
    for name, m, inside in tc.bil_range_cases():
        base = m[0, 0]  # every range case leaves the map's first pixel at its base value
        _check_condition(name, inside, f(m), f(tc.uniform(tc.STD_H, tc.STD_W, base)))
        span = float(m.max() - m.min())
        assert span == (tc.BIL_D if "span%d_" % tc.BIL_D in name else tc.BIL_D - 1), name
        assert np.abs(m).max() < tc.LIMIT and np.array_equal(m, np.floor(m))
    # a range of D against D - 1 is a different result (the clamped LUT index), not the same one reached another way
    a, (y, x) = 0.0, (tc.Y0 - R, tc.X0 - R)
    m0, m1 = tc.uniform(tc.STD_H, tc.STD_W, a), tc.uniform(tc.STD_H, tc.STD_W, a)
    m0[y, x], m1[y, x] = a + tc.BIL_D - 1, a + tc.BIL_D
    assert f(m0)[tc.Y0, tc.X0] != f(m1)[tc.Y0, tc.X0]


@pytest.mark.parametrize("cfg", tc.TABLE_CONFIGS, ids=["%dx%d_D%d_zd%d" % c for c in tc.TABLE_CONFIGS])
def test_every_table_entry_is_reached_in_both_views(orc, cfg):
    """no entry left out: for every v the map entering the bilateral filter has a block whose scanned region holds only v"""
    H, W, D, zd = cfg
    frames = tc.table_frames(orc, cfg)
    assert sorted(frames) == list(range(-zd, D - zd)) and len(frames) == D
    for v, (_, _, _, voted_l, voted_r) in frames.items():
        for side, m in (("left", voted_l), ("right", voted_r)):
            assert m.shape == (H, W)
            n = sum(1 for _, _, val in tc.one_value_blocks(m, tc.BIL[0]) if val == float(v))
            assert n >= 1, (v, side)
    assert set(tc.table_stage3_values(cfg)) == {-zd, 0, D - 1 - zd}
