"""The stencil kernels' tile forms on the GPU, bit for bit against the CPU oracle on the directed maps of tests/tile_cases.py:
stm_k_gaussian_max_r's one-value form (per stage, and inverted through dibr_dbm), stm_k_bilateral_r<7, true>'s integer, one-value
and general forms (per stage under stm_set_agg_variant(500), null table: the wave-computed number), and every entry of the
host-built one-value table through the frame.  What makes a case worth running is asserted on the oracle in
test_tile_shortcuts_ref.py; here every output is compared with the oracle's, whole map, exact equality."""
import numpy as np
import pytest

import tile_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(gpu_ready):
    from stm_amd import host_api
    return host_api


def _same(got, want, name):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want)))) if got.dtype.kind == "f" else np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d elements differ from the oracle, the first at %s (%r, oracle %r)" % (
        name, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _device_flavour(fn, m, *args):
    """a device-flavour in-place filter (stm_d_filter_*_1(d_img, ..., num_rows, num_cols, ...)) on a copy of m; args: the
    arguments before and after the shape, the shape's place marked by None"""
    import torch
    from stm_amd import device_api as dev
    t = torch.from_numpy(m.copy()).cuda()
    k = args.index(None)
    dev._use_current_stream()
    fn(dev._p(t), *args[:k], m.shape[0], m.shape[1], *args[k + 1:])
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ----------------------------------------------------------------------------- A
@pytest.mark.parametrize("R,sigma", tc.GAUSS_FAST + [tc.GAUSS_GENERIC])
def test_gaussian_forms(api, orc, stm, R, sigma):
    """Uniform maps (0 and 1 are stored, 0.5, 2 and -1 must not be), one raised pixel on and around every edge of the middle block's
    needed neighbourhood, the mixed maps and the edge shapes; radius 3 runs the generic kernel on the same maps.  Host flavour
    throughout, the device flavour on the uniform maps, the corners, one pixel per edge and the mixed map."""
    corners = {"y%d_x%d" % p for p in [(tc.Y0 - R, tc.X0 - R), (tc.Y0 + 15 + R, tc.X0 + 63 + R), (tc.Y0 + 5, tc.X0 + 63 + R),
                                       (tc.Y0 + 5, tc.X0 + 64 + R), (tc.Y0 + 15 + R, tc.X0 + 9), (tc.Y0 - R, tc.X0 + 9),
                                       (tc.Y0 + 5, tc.X0 - R)]}
    n = nd = 0
    for name, m, _ in tc.gauss_cases(R):
        want = orc.filter_gaussian_1(m, R, sigma)
        _same(api.filter_gaussian_1(m, R, sigma), want, name)
        n += 1
        if name.startswith("uniform") or name == "mixed" or name.split("_", 2)[-1] in corners:
            _same(_device_flavour(stm.lib().stm_d_filter_gaussian_1, m, R, sigma, None), want, name + " (device flavour)")
            nd += 1
    assert n > 150 and nd >= 5 + 1 + 2 * len(corners)


# ----------------------------------------------------------------------------- B
def _dbm_device(il, ir, dl, dr, ml, mr, shift):
    import torch
    from stm_amd import device_api as dev
    H, W, E = il.shape
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (il, ir, dl, dr, ml, mr)]
    out = torch.zeros(H, W, E, dtype=torch.uint8, device="cuda")
    dev._use_current_stream()
    dev.lib().stm_d_dibr_dbm(dev._p(out), dev._p(t[0]), dev._p(t[1]), dev._p(t[2]), dev._p(t[3]), None, None, dev._p(t[4]),
                             dev._p(t[5]), float(shift), H, W, E)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("flavour", ["host", "device"])
def test_gaussian_inverted_form_through_dbm(api, orc, flavour):
    """core_dbm blurs 1 - mask_r with the same kernel (invert = 1): uniform masks, and a line on the outermost needed halo row /
    column of the middle block and one beyond it.  The host flavour blurs with (7, 10), the device flavour with (10, 15), so
    each has its own lines."""
    R, sigma = (7, 10.0) if flavour == "host" else (10, 15.0)
    il, ir, dl, dr, ml = tc.dbm_inputs()
    occl = np.zeros(ml.shape, np.uint8)
    n = 0
    for name, mr, _ in tc.dbm_cases(R):
        want = orc.dibr_dbm(il, ir, dl, dr, ml, mr, tc.DBM_SHIFT, R, sigma)
        if flavour == "host":
            got = api.dibr_dbm(il, ir, dl, dr, occl, occl, ml, mr, tc.DBM_SHIFT)
        else:
            got = _dbm_device(il, ir, dl, dr, ml, mr, tc.DBM_SHIFT)
        _same(got, want, name)
        n += 1
    assert n == 18


# ----------------------------------------------------------------------------- C
def test_bilateral_forms(api, orc, stm):
    """stm_k_bilateral_r<7, true> on the caller's map (variant 500, null table): uniform maps up to the limits of the integer
    form, one pixel c + 1 (integer form next to one-value blocks) and c + 0.5 (general form) around the middle block's needed
    neighbourhood, ranges of exactly D - 1 and D, the edge shapes; a subset through the device flavour.  The default variant's
    general-form kernel runs the uniform and the range maps as a cross-check."""
    R, sc, ss = tc.BIL
    lib = stm.lib()
    cases = list(tc.bil_cases())
    want = [orc.filter_bilateral_1(m, R, sc, ss, tc.BIL_D) for _, m, _ in cases]
    lib.stm_set_agg_variant(500)
    try:
        for (name, m, _), w in zip(cases, want):
            _same(api.filter_bilateral_1(m, R, sc, ss, tc.BIL_D), w, name)
            if name.startswith("uniform") or "span" in name:
                _same(_device_flavour(lib.stm_d_filter_bilateral_1, m, R, sc, ss, None, tc.BIL_D), w, name + " (device flavour)")
    finally:
        lib.stm_set_agg_variant(0)
    for (name, m, _), w in zip(cases, want):
        if name.startswith("uniform") or "span" in name:
            _same(api.filter_bilateral_1(m, R, sc, ss, tc.BIL_D), w, name + " (default variant)")
    assert len(cases) > 250


# ----------------------------------------------------------------------------- D
def _run_frame(sbs, p, stages, H, W):
    import torch
    from stm_amd import device_api as dev
    d_sbs = torch.from_numpy(sbs.copy()).cuda()
    dl = torch.full((H, W), -777.0, dtype=torch.float32, device="cuda")
    dr = torch.full_like(dl, -777.0)
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("cfg", tc.TABLE_CONFIGS, ids=["%dx%d_D%d_zd%d" % c for c in tc.TABLE_CONFIGS])
def test_every_entry_of_the_one_value_table_through_the_frame(gpu_ready, orc, cfg):
    """Only the frame pipeline passes bilateral_one_value_table to the kernel.  A pair with the constant shift -v gives maps with
    whole blocks of v (test_tile_shortcuts_ref.py: at least one per view, for every v), so the frame's disparity maps hold entry
    v + zd of the table there: all D entries of four (D, zd) are compared with the oracle's filter, and the first, the last and
    the entry of v = 0 once more through the whole frame."""
    from stm_amd import device_api as dev
    H, W, D, zd = cfg
    p = dev.FrameParams(num_disp=D, zero_disp=zd, usd=tc.TABLE_USD, lsd=tc.TABLE_LSD)
    q = tc.Params(D, zd)
    assert all(getattr(p, k) == getattr(q, k) for k in vars(q)), "tile_cases.Params is not FrameParams' defaults any more"
    for v, (sbs, want_l, want_r, _, _) in tc.table_frames(orc, cfg).items():
        dl, dr, _ = _run_frame(sbs, p, 2, H, W)
        _same(dl, want_l, "v = %d, disp_l" % v)
        _same(dr, want_r, "v = %d, disp_r" % v)
    for v in tc.table_stage3_values(cfg):
        want_l, want_r, want_mux = tc.table_frame3(orc, cfg, v)
        dl, dr, mux = _run_frame(tc.table_pair(cfg, v), p, 3, H, W)
        _same(dl, want_l, "v = %d, stages = 3, disp_l" % v)
        _same(dr, want_r, "v = %d, stages = 3, disp_r" % v)
        _same(mux, want_mux, "v = %d, interlaced" % v)
