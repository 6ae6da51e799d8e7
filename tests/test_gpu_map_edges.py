"""The map-taking stages on huge and non-finite disparities, on the GPU: dr_dcc, dibr_occl, dibr_dfm, dr_irv, filter_bilateral_1 and
filter_median in host and device flavour on the cases of tests/map_edge_cases.py, every output equal to the oracle's (floats with
NaNs compared by position) and every input left as it was, bit for bit.  The rules are in include/stm_hip.h ("Map values a stage
cannot place"); test_map_edges_ref.py shows on the oracle that a kernel which adds a saturated conversion to a coordinate in a
32-bit register gives another result on these cases.  dibr_dbm / dibr_dbm_lin are not here: test_gpu_linwarp.py runs both samplers
on NaN, +-inf and far positions."""
import numpy as np
import pytest

import map_edge_cases as mc
from map_edge_cases import same

pytestmark = pytest.mark.gpu
SHIFTS = [0.0, 0.4, 1.0, -1.0]


@pytest.fixture(scope="module")
def api(gpu_ready):
    from stm_amd import host_api
    return host_api


@pytest.fixture(scope="module")
def dev(gpu_ready):
    from stm_amd import device_api
    return device_api


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint8).copy()


def _stack(arrs):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack(arrs))).cuda()


def _unchanged(t, arrs):
    """the device copies of the inputs still hold the cases' bits"""
    return np.array_equal(_bits(t.cpu().numpy()), _bits(np.stack(arrs)))


def _report(stage, bad):
    """every failing case and its count of differing elements in one message: the first GPU run's record reads from it"""
    assert not bad, "%s: %d runs differ from the oracle, %d elements in all; the first: %s" % (
        stage, len(bad), sum(n for _, n in bad), bad[:6])


def _diff(got, want):
    if got.dtype.kind == "f":
        return int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())
    return int((got != want).sum())


@pytest.mark.parametrize("H,W", mc.SHAPES)
def test_dcc_and_occl(api, dev, orc, stm, H, W):
    """both outlier planes of dr_dcc and both hit maps of dibr_occl"""
    import torch
    lib = stm.lib()
    cases = mc.pair_cases(H, W)
    tl, tr = _stack([c[1] for c in cases]), _stack([c[2] for c in cases])
    for stage, host, d_fn, ref in (("dr_dcc", api.dr_dcc, lib.stm_d_dr_dcc, orc.dr_dcc),
                                   ("dibr_occl", api.dibr_occl, lib.stm_d_dibr_occl, orc.dibr_occl)):
        out = torch.zeros(2, len(cases), H, W, dtype=torch.uint8, device="cuda")   # device flavour: zero-filled by the caller
        dev._use_current_stream()
        for n in range(len(cases)):
            d_fn(dev._p(out[0, n]), dev._p(out[1, n]), dev._p(tl[n]), dev._p(tr[n]), H, W)
        torch.cuda.synchronize()
        got_d = out.cpu().numpy()
        bad = []
        for n, (name, dl, dr, _) in enumerate(cases):
            bl, br = _bits(dl), _bits(dr)
            want = ref(dl, dr)
            got = host(dl, dr)
            assert np.array_equal(_bits(dl), bl) and np.array_equal(_bits(dr), br), (stage, name, "inputs modified")
            for flavour, g in (("host", got), ("device", (got_d[0, n], got_d[1, n]))):
                k = _diff(g[0], want[0]) + _diff(g[1], want[1])
                if k:
                    bad.append(("%s %s" % (name, flavour), k))
        _report(stage, bad)
    assert _unchanged(tl, [c[1] for c in cases]) and _unchanged(tr, [c[2] for c in cases])


@pytest.mark.parametrize("H,W", mc.SHAPES)
def test_dfm(api, dev, orc, stm, H, W):
    """shifts 0, 0.4, 1 and -1 (the f32 product of an infinite value and 0 is a NaN), 3 and 4 bytes per pixel"""
    import torch
    lib = stm.lib()
    cases = mc.pair_cases(H, W)
    tl, tr = _stack([c[1] for c in cases]), _stack([c[2] for c in cases])
    bad = []
    for E in (3, 4):
        il, ir = mc.images(H, W, E)
        til, tir = torch.from_numpy(il.copy()).cuda(), torch.from_numpy(ir.copy()).cuda()
        for shift in SHIFTS:
            out = torch.zeros(len(cases), H, W, E, dtype=torch.uint8, device="cuda")
            dev._use_current_stream()
            for n in range(len(cases)):
                lib.stm_d_dibr_dfm(dev._p(out[n]), dev._p(til), dev._p(tir), dev._p(tl[n]), dev._p(tr[n]), shift, H, W, E)
            torch.cuda.synchronize()
            got_d = out.cpu().numpy()
            for n, (name, dl, dr, _) in enumerate(cases):
                want = orc.dibr_dfm(il, ir, dl, dr, shift)
                for flavour, g in (("host", api.dibr_dfm(il, ir, dl, dr, shift)), ("device", got_d[n])):
                    k = _diff(g, want)
                    if k:
                        bad.append(("%s shift %g elem_sz %d %s" % (name, shift, E, flavour), k))
        assert np.array_equal(til.cpu().numpy(), il) and np.array_equal(tir.cpu().numpy(), ir)
    _report("dibr_dfm", bad)
    assert _unchanged(tl, [c[1] for c in cases]) and _unchanged(tr, [c[2] for c in cases])


@pytest.mark.parametrize("H,W", mc.SHAPES)
def test_median(api, dev, orc, stm, H, W):
    """the first comparison of stm_k_median3 with the conversion it states: NaN -> 0, saturation at both ends"""
    import torch
    lib = stm.lib()
    cases = mc.pair_cases(H, W)
    maps = [c[1] for c in cases] + [c[2] for c in cases]
    t = _stack(maps)
    dev._use_current_stream()
    for n in range(len(maps)):
        lib.stm_d_filter_median(dev._p(t[n]), H, W)   # in place
    torch.cuda.synchronize()
    got_d = t.cpu().numpy()
    bad = []
    for n, m in enumerate(maps):
        before = _bits(m)
        want = orc.filter_median(m)
        got = api.filter_median(m)
        assert np.array_equal(_bits(m), before)
        for flavour, g in (("host", got), ("device", got_d[n])):
            k = _diff(g, want)
            if k:
                bad.append(("%s %s %s" % (cases[n % len(cases)][0], "lr"[n // len(cases)], flavour), k))
    _report("filter_median", bad)


@pytest.mark.parametrize("variant,radius,sc,ss", [(0, 7, 5.0, 10.0), (500, 7, 5.0, 10.0), (0, 2, 1.5, 1.0)])
@pytest.mark.parametrize("H,W", mc.SHAPES)
def test_bilateral(api, dev, orc, stm, H, W, variant, radius, sc, ss):
    """radius 7 in the default form and as stm_k_bilateral_r<7, true> (stm_set_agg_variant(500)), and radius 2: a NaN difference
    takes table entry 0, an infinite one entry D - 1"""
    import torch
    lib = stm.lib()
    cases = mc.pair_cases(H, W, whole=True)
    maps = [c[1] for c in cases]
    bad = []
    lib.stm_set_agg_variant(variant)
    try:
        t = _stack(maps)
        dev._use_current_stream()
        for n in range(len(maps)):
            lib.stm_d_filter_bilateral_1(dev._p(t[n]), radius, sc, ss, H, W, mc.BIL_D)
        torch.cuda.synchronize()
        got_d = t.cpu().numpy()
        for n, m in enumerate(maps):
            before = _bits(m)
            want = orc.filter_bilateral_1(m, radius, sc, ss, mc.BIL_D)
            got = api.filter_bilateral_1(m, radius, sc, ss, mc.BIL_D)
            assert np.array_equal(_bits(m), before)
            for flavour, g in (("host", got), ("device", got_d[n])):
                k = _diff(g, want)
                if k:
                    bad.append(("%s %s" % (cases[n][0], flavour), k))
    finally:
        lib.stm_set_agg_variant(0)
    _report("filter_bilateral_1 radius %d variant %d" % (radius, variant), bad)


def _irv_runs(api, dev, orc, stm, H, W, D, zd, iterations, params, every=1):
    """dr_irv in both flavours on the shape's cases -> the runs that differ from the oracle"""
    import torch
    lib = stm.lib()
    cases = mc.irv_cases(orc, H, W, D, zd)[::every]
    cross = cases[0][4]
    tx = torch.from_numpy(cross.copy()).cuda()
    tab = dev.plane_table(tx)
    bad = []
    for ts, th in params:
        td, to = _stack([c[2] for c in cases]), _stack([c[3] for c in cases])
        dev._use_current_stream()
        for n in range(len(cases)):
            lib.stm_d_dr_irv(dev._p(td[n]), dev._p(to[n]), dev._p(tab), ts, th, H, W, D, zd, mc.USD, iterations)
        torch.cuda.synchronize()
        gd, go = td.cpu().numpy(), to.cpu().numpy()
        for n, (name, _, disp, outl, _, _) in enumerate(cases):
            bd, bo, bx = _bits(disp), _bits(outl), _bits(cross)
            for flavour, got in (("host", api.dr_irv(disp, outl, cross, ts, th, D, zd, mc.USD, iterations)), ("device", (gd[n], go[n]))):
                want = orc.dr_irv(disp, outl, cross, ts, th, D, zd, mc.USD, iterations, device_flavour=(flavour == "device"))
                k = _diff(got[0], want[0]) + _diff(got[1], want[1])
                if k:
                    bad.append(("%s thresh_s %d thresh_h %g %s" % (name, ts, th, flavour), k))
            assert np.array_equal(_bits(disp), bd) and np.array_equal(_bits(outl), bo) and np.array_equal(_bits(cross), bx), name
    assert np.array_equal(tx.cpu().numpy(), cross)
    assert b"outlier list" not in (lib.stm_last_error() or b"")
    return bad


@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("D,zd", mc.IRV_RANGES)
@pytest.mark.parametrize("H,W", mc.SHAPES)
def test_irv(api, dev, orc, stm, H, W, D, zd, iterations):
    """the map and the outliers; planted values that vote, that are an outlier's own value, and outliers in whose region nothing has
    a bin, so that the winner is f2i_sat(own) and the accept ratio's numerator f2i_sat(own) + zd, a sum beyond 32 bits"""
    bad = _irv_runs(api, dev, orc, stm, H, W, D, zd, iterations, [(0, 0.0), (4, 0.0), (0, 0.1), (4, 0.1)])
    _report("dr_irv D %d zd %d, %d iterations" % (D, zd, iterations), bad)


def test_irv_paper_ratio(api, dev, orc, stm):
    """stm_set_irv_paper_ratio(1): the numerator is the winning bin's count, so no sum with `own` enters the accept test"""
    lib = stm.lib()
    lib.stm_set_irv_paper_ratio(1)
    orc.set_irv_paper_ratio(1)
    try:
        bad = _irv_runs(api, dev, orc, stm, 9, 37, 8, 4, 3, [(0, 0.1)])
    finally:
        lib.stm_set_irv_paper_ratio(0)
        orc.set_irv_paper_ratio(0)
    _report("dr_irv, paper ratio", bad)
