"""The cases on which the reference's own kernels (oracle/_ref/libstm_ref_hip.so, see oracle/build_ref.py) are compared
with the oracle and the HIP library, shared by

  tests/test_gpu_reference.py        reference (child process, MI355X) vs oracle vs HIP library, same input arrays
  tests/golden/make_golden_ref.py    records the reference's outputs on the MI355X into tests/golden/ref_gfx950_*.npz
  tests/test_oracle_vs_reference.py  oracle vs those recorded outputs, on any machine

Every case is one stage call: (name, stage, parameters, builder of the input arrays).  The builders use only committed
fixtures (bud / fish), conftest.rand_pair, synth frames and the oracle for upstream stages, so the same arrays come out
everywhere.  Every shape is inside the reference's launch envelope (oracle/pyref.admit asserts it).

Rules of comparison (RULES): "exact" = equal element for element, NaNs at the same places; "tol" = absolute difference
at most TOL[stage].  TOL is four times the maximum |reference - oracle| measured on the MI355X over all cases of the
stage (profiles/ref_parity.json), and never above 1e-4, the bound SURVEY A-Q18 / the north star set.
"""
import json
import os
import subprocess
import sys
import zlib

import numpy as np

from conftest import GOLDEN, ROOT, rand_pair

FLT_MAX = np.finfo(np.float32).max
BOUND = 1e-4

# measured maxima of |reference - oracle| on the MI355X (profiles/ref_parity.json) -> tolerance = min(4 * max, 1e-4)
MEASURED_MAX = {"ci_adcensus": 2.384185791015625e-07, "filter_bilateral_1": 0.0}
TOL = {k: min(4.0 * v, BOUND) for k, v in MEASURED_MAX.items()}

RULES = {
    "ci_adcensus": {"cost_l": "tol", "cost_r": "tol"},
    "ca_cross": {"cross": "exact", "acost": "exact"},
    "dc_wta": {"disp": "exact"},
    "dr_dcc": {"outliers_l": "exact", "outliers_r": "exact"},
    "filter_bilateral_1": {"img": "tol"},
    "filter_gaussian_1": {"img": "exact"},
    "filter_bleed_1": {"img": "exact"},
    "dibr_occl": {"occl_l": "exact", "occl_r": "exact"},
    "dibr_occl_to_mask": {"mask_l": "exact", "mask_r": "exact"},
    "dibr_dbm": {"view": "exact"},
    "mux_multiview": {"out": "exact"},
    "tx_scale": {"out": "exact"},
}

AD, CE, UCD, LCD = 10.0, 30.0, 6.0, 20.0


def _bmp(name):
    from stm_amd import bmp_io
    return bmp_io.read_bmp(os.path.join(GOLDEN, name + ".bmp"))


def _crop(img, y0, x0, H, W):
    return np.ascontiguousarray(img[y0:y0 + H, x0:x0 + W])


def pair(kind, H, W):
    """An input pair: 'bud' / 'fish' crops of the committed fixtures, 'rand' = conftest.rand_pair, 'synth' = a synthetic
    side-by-side frame with known disparities."""
    if kind == "bud_full":
        return _crop(_bmp("bud_2"), 0, 0, H, W), _crop(_bmp("bud_3"), 0, 0, H, W)
    if kind == "bud":
        return _crop(_bmp("bud_2"), 150, 160, H, W), _crop(_bmp("bud_3"), 150, 160, H, W)
    if kind == "fish":
        return _crop(_bmp("fish_1"), 96, 160, H, W), _crop(_bmp("fish_2"), 96, 160, H, W)
    if kind == "synth":
        from stm_amd import synth
        sbs, _ = synth.sbs_frame(H, W, 16, 8)
        return np.ascontiguousarray(sbs[:, :W]), np.ascontiguousarray(sbs[:, W:2 * W])
    return rand_pair(H, W, 1000 + H + W)


def _disp_pair(orc, kind, H, W, D, zd, usd=17, lsd=8):
    """WTA maps of both views from the oracle's own chain (integer valued, inside [-zd, D-1-zd])."""
    L, R = pair(kind, H, W)
    cl, cr = orc.ci_adcensus(L, R, AD, CE, D, zd)
    dl = orc.dc_wta(orc.ca_cross(L, cl, UCD, LCD, usd, lsd)[1], zd)
    dr = orc.dc_wta(orc.ca_cross(R, cr, UCD, LCD, usd, lsd)[1], zd)
    return L, R, dl, dr


def _b_ci(kind, H, W):
    def build(orc, p):
        L, R = pair(kind, H, W)
        return {"img_l": L, "img_r": R}
    return build


def _b_agg(kind, H, W, special=None):
    def build(orc, p):
        L, R = pair(kind, H, W)
        D = p["D"]
        cost, _ = orc.ci_adcensus(L, R, AD, CE, D, D // 2)
        cost = cost.copy()
        if special == "fltmax_run":
            # a run of FLT_MAX markers inside one window (their sum overflows to +inf in the first pass), a lone marker, and a
            # vertical pair; everything else ordinary
            cost[1, H // 2, W // 2:W // 2 + 3] = FLT_MAX
            cost[D - 1, 5, 7] = FLT_MAX
            cost[0, H - 9:H - 7, W - 11] = FLT_MAX
        elif special == "inf":
            cost[2, H // 3, W // 3] = np.inf
            cost[0, 3, W - 4] = -np.inf
            cost[D - 2, H - 5, 9] = np.nan
            cost[3, H // 2, 40:42] = FLT_MAX
        return {"img": L, "cost": cost}
    return build


def _b_wta(kind, H, W):
    def build(orc, p):
        if kind == "ties":  # small-integer costs: most pixels have several equal minima, the lowest d must win (A-Q13)
            rs = np.random.RandomState(77)
            return {"cost": rs.randint(0, 3, size=(p["D"], H, W)).astype(np.float32)}
        L, R = pair(kind, H, W)
        cl, _ = orc.ci_adcensus(L, R, AD, CE, p["D"], p["zd"])
        return {"cost": orc.ca_cross(L, cl, UCD, LCD, 17, 8)[1]}
    return build


def _b_disp(kind, H, W, D=16, zd=8):
    def build(orc, p):
        if kind == "frac":  # fractional maps: the (int) truncation toward zero of A-Q16 / A-Q19 on both signs
            rs = np.random.RandomState(H + W)
            dl = (rs.randint(-7, 7, size=(H, W)) + rs.random_sample((H, W)) * 0.9).astype(np.float32)
            dr = (rs.randint(-7, 7, size=(H, W)) + rs.random_sample((H, W)) * 0.9).astype(np.float32)
            dl[::5, ::3] = np.round(dl[::5, ::3])
            return {"disp_l": dl, "disp_r": dr}
        if kind == "edges":
            # the fractional maps with NaN and values far beyond the row planted in both: every one with |v| < 2^31 - W, so that
            # x + (int)v and x - (int)v overflow in nobody's 32 bits, the reference's included (it clamps the column after the
            # sum, d_dr_dcc.cu:45-51, :69-76, d_dibr_occl.cu:124-125).  Pins "NaN -> 0, truncate toward zero" to its binary.
            a = _b_disp("frac", H, W)(orc, p)
            vals = np.array([np.nan, 2147483520.0, -2147483520.0, 1e9, -1e9, W, -W, W - 1, -(W - 1), W + 0.5, -(W + 0.5), 0.999,
                             -0.999, -0.0, 1e-40, -1e-40], np.float32)
            assert all(abs(float(v)) < 2 ** 31 - W for v in vals[1:])
            rs = np.random.RandomState(3 * H + W)
            for m in (a["disp_l"], a["disp_r"]):
                cols = [0, 1, W // 2, W - 2, W - 1] + rs.randint(2, W - 2, size=3 * len(vals)).tolist()
                for j, c in enumerate(cols):
                    m[(5 * j + 1) % H, c] = vals[j % len(vals)]
                m[H - 1, :len(vals)] = vals          # and side by side, so that neighbours' targets collide
            return a
        _, _, dl, dr = _disp_pair(orc, kind, H, W, D, zd)
        return {"disp_l": dl, "disp_r": dr}
    return build


def _b_bilateral(kind, H, W):
    def build(orc, p):
        D = p["D"]
        if kind == "steps":  # integer steps of every height below D next to each other: every colour-table entry is used
            rs = np.random.RandomState(5)
            img = np.kron(rs.randint(0, D, size=(H // 6, W // 8)), np.ones((6, 8))).astype(np.float32) - D // 2
            return {"img": img}
        _, _, dl, _ = _disp_pair(orc, kind, H, W, D, D // 2)
        return {"img": dl}
    return build


def _b_mask(H, W, thr, seed):
    def build(orc, p):
        rs = np.random.RandomState(seed)
        return {"img": (rs.random_sample((H, W)) > thr).astype(np.float32)}
    return build


def _b_bleed(H, W, thr, seed):
    def build(orc, p):
        rs = np.random.RandomState(seed)
        return {"img": (rs.random_sample((H, W)) > thr).astype(np.uint8)}
    return build


def _b_occl_mask(H, W):
    def build(orc, p):
        _, _, dl, dr = _disp_pair(orc, "rand", H, W, 16, 8)
        ol, orr = orc.dibr_occl(dl, dr)
        return {"occl_l": orc.filter_bleed_1(ol, 1), "occl_r": orc.filter_bleed_1(orr, 1)}
    return build


def _dbm_inputs(orc, kind, H, W):
    L, R, dl, dr = _disp_pair(orc, kind, H, W, 16, 8)
    if kind == "rand":  # fractional disparities as the bilateral leaves them
        dl = orc.filter_bilateral_1(dl, 7, 5.0, 10.0, 16)
        dr = orc.filter_bilateral_1(dr, 7, 5.0, 10.0, 16)
    ol, orr = orc.dibr_occl(dl, dr)
    ol, orr = orc.filter_bleed_1(ol, 1), orc.filter_bleed_1(orr, 1)
    ml, mr = orc.dibr_occl_to_mask(ol, orr)
    return {"img_l": L, "img_r": R, "disp_l": dl, "disp_r": dr, "occl_l": ol, "occl_r": orr, "mask_l": ml, "mask_r": mr}


def _b_dbm(kind, H, W):
    def build(orc, p):
        return _dbm_inputs(orc, kind, H, W)
    return build


def view_shift(v, N=8):
    return float(np.float32(1.0 - (1.0 * np.float32(v)) / (np.float32(N) - 1.0)))


def _b_mux(kind, H, W):
    def build(orc, p):
        a = _dbm_inputs(orc, kind, H, W)
        views = [a["img_r"]]
        for v in range(1, 7):
            views.append(orc.dibr_dbm(a["img_l"], a["img_r"], a["disp_l"], a["disp_r"], a["mask_l"], a["mask_r"], view_shift(v), 7, 10.0))
        views.append(a["img_l"])
        return {"views": np.stack(views)}
    return build


def _b_img(kind, H, W):
    def build(orc, p):
        return {"img": pair(kind, H, W)[0]}
    return build


def _ci(D, zd):
    return {"ad_coeff": AD, "census_coeff": CE, "D": D, "zd": zd}


def _agg(D, usd, lsd):
    return {"ucd": UCD, "lcd": LCD, "usd": usd, "lsd": lsd, "D": D}


CASES = [
    # cost init: W % 160 == 0 (A-L4); zd on both sides of D - zd <= zd (AD strays of A-Q7 only on the first side)
    ("ci_rand_160x32_D16_zd8", "ci_adcensus", _ci(16, 8), _b_ci("rand", 32, 160)),
    ("ci_bud_320x32_D24_zd6", "ci_adcensus", _ci(24, 6), _b_ci("bud", 32, 320)),
    ("ci_fish_160x64_D9_zd7", "ci_adcensus", _ci(9, 7), _b_ci("fish", 64, 160)),
    ("ci_synth_320x32_D16_zd8", "ci_adcensus", _ci(16, 8), _b_ci("synth", 32, 320)),
    # arms + aggregation on an oracle-made volume: W % 32 == 0, H % 32 == 0 (A-L3); lsd < usd and lsd == usd
    ("agg_rand_160x64_D8_usd17_lsd8", "ca_cross", _agg(8, 17, 8), _b_agg("rand", 64, 160)),
    ("agg_bud_320x96_D6_usd9_lsd9", "ca_cross", _agg(6, 9, 9), _b_agg("bud", 96, 320)),
    ("agg_fish_96x32_D5_usd34_lsd17", "ca_cross", _agg(5, 34, 17), _b_agg("fish", 32, 96)),
    ("agg_rand_160x64_D8_fltmax_run", "ca_cross", _agg(8, 17, 8), _b_agg("rand", 64, 160, "fltmax_run")),
    ("agg_bud_96x64_D6_inf_nan", "ca_cross", _agg(6, 34, 17), _b_agg("bud", 64, 96, "inf")),
    # winner takes all, with ties
    ("wta_bud_320x32_D24_zd6", "dc_wta", {"D": 24, "zd": 6}, _b_wta("bud", 32, 320)),
    ("wta_ties_64x48_D11_zd4", "dc_wta", {"D": 11, "zd": 4}, _b_wta("ties", 48, 64)),
    # left-right check classes
    ("dcc_bud_160x64", "dr_dcc", {}, _b_disp("bud", 64, 160)),
    ("dcc_frac_96x32", "dr_dcc", {}, _b_disp("frac", 32, 96)),
    ("dcc_edges_96x32", "dr_dcc", {}, _b_disp("edges", 32, 96)),   # NaN and |v| up to 2147483520 in both maps
    # bilateral: H % 30 == 0, W % 32 == 0 (A-L6); value range below D (A-Q18)
    ("bil_bud_160x60_D16", "filter_bilateral_1", {"radius": 7, "sigma_color": 5.0, "sigma_spatial": 10.0, "D": 16}, _b_bilateral("bud", 60, 160)),
    ("bil_steps_64x90_D32", "filter_bilateral_1", {"radius": 7, "sigma_color": 5.0, "sigma_spatial": 10.0, "D": 32}, _b_bilateral("steps", 90, 64)),
    ("bil_rand_96x30_D16_r3", "filter_bilateral_1", {"radius": 3, "sigma_color": 2.0, "sigma_spatial": 4.0, "D": 16}, _b_bilateral("rand", 30, 96)),
    # grow-only gaussian of a mask, bleed
    ("gauss_96x64_r10", "filter_gaussian_1", {"radius": 10, "sigma": 15.0}, _b_mask(64, 96, 0.8, 4)),
    ("gauss_160x32_r7", "filter_gaussian_1", {"radius": 7, "sigma": 10.0}, _b_mask(32, 160, 0.6, 5)),
    ("bleed_96x64_r1", "filter_bleed_1", {"radius": 1}, _b_bleed(64, 96, 0.7, 6)),
    ("bleed_64x32_r2", "filter_bleed_1", {"radius": 2}, _b_bleed(32, 64, 0.8, 7)),
    # hit maps and mask
    ("occl_bud_160x64", "dibr_occl", {}, _b_disp("bud", 64, 160)),
    ("occl_frac_96x32", "dibr_occl", {}, _b_disp("frac", 32, 96)),
    ("occl_edges_96x32", "dibr_occl", {}, _b_disp("edges", 32, 96)),
    ("mask_160x32", "dibr_occl_to_mask", {}, _b_occl_mask(32, 160)),
    ("mask_96x64", "dibr_occl_to_mask", {}, _b_occl_mask(64, 96)),
    # backward warp + invert + gaussian-max + merge (host flavour: gaussian(7, 10)), two shifts, integer and fractional maps
    ("dbm_bud_160x64_v2", "dibr_dbm", {"shift": view_shift(2)}, _b_dbm("bud", 64, 160)),
    ("dbm_rand_96x32_v5", "dibr_dbm", {"shift": view_shift(5)}, _b_dbm("rand", 32, 96)),
    # interlacing: the strided kernel (Hout % N == 0, Wout % N == 0) and the general one (Hout % N != 0)
    ("mux_bud_160x64_to_320x128", "mux_multiview", {"angle": 18.43, "Hout": 128, "Wout": 320}, _b_mux("bud", 64, 160)),
    ("mux_rand_96x32_to_100x35", "mux_multiview", {"angle": 18.0, "Hout": 35, "Wout": 100}, _b_mux("rand", 32, 96)),
    # bilinear resize, down and up, ragged output sizes
    ("scale_bud_160x64_to_70x30", "tx_scale", {"Hout": 30, "Wout": 70}, _b_img("bud", 64, 160)),
    ("scale_rand_96x32_to_200x75", "tx_scale", {"Hout": 75, "Wout": 200}, _b_img("rand", 32, 96)),
]
CASE_IDS = [c[0] for c in CASES]

# Compared on the MI355X only (too large to record): the reference's own bud pair at its own size, 640 x 384, which its launch
# geometry covers for these stages (640 = 4 x 160 = 20 x 32, 384 = 12 x 32), with the parameters of its image program.
GPU_ONLY_CASES = [
    ("ci_bud_640x384_D32_zd16", "ci_adcensus", _ci(32, 16), _b_ci("bud_full", 384, 640)),
    ("agg_bud_640x384_D32_usd17_lsd8", "ca_cross", _agg(32, 17, 8), _b_agg("bud_full", 384, 640)),
    ("wta_bud_640x384_D32_zd16", "dc_wta", {"D": 32, "zd": 16}, _b_wta("bud_full", 384, 640)),
]


def run_oracle(orc, stage, p, a, quirks=True):
    """The oracle on the case's inputs, outputs named as oracle/pyref.run_call names the reference's.  Cost init runs in
    ref_quirks mode (A-Q7: the reference's stray tile reads at d = 0) unless quirks=False."""
    if stage == "ci_adcensus":
        orc.set_ref_quirks(1 if quirks else 0)
        try:
            cl, cr = orc.ci_adcensus(a["img_l"], a["img_r"], p["ad_coeff"], p["census_coeff"], p["D"], p["zd"])
        finally:
            orc.set_ref_quirks(0)
        return {"cost_l": cl, "cost_r": cr}
    if stage == "ca_cross":
        cross, acost = orc.ca_cross(a["img"], a["cost"], p["ucd"], p["lcd"], p["usd"], p["lsd"])
        return {"cross": cross, "acost": acost}
    if stage == "dc_wta":
        return {"disp": orc.dc_wta(a["cost"], p["zd"])}
    if stage == "dr_dcc":
        ol, orr = orc.dr_dcc(a["disp_l"], a["disp_r"])
        return {"outliers_l": ol, "outliers_r": orr}
    if stage == "filter_bilateral_1":
        return {"img": orc.filter_bilateral_1(a["img"], p["radius"], p["sigma_color"], p["sigma_spatial"], p["D"])}
    if stage == "filter_gaussian_1":
        return {"img": orc.filter_gaussian_1(a["img"], p["radius"], p["sigma"])}
    if stage == "filter_bleed_1":
        return {"img": orc.filter_bleed_1(a["img"], p["radius"])}
    if stage == "dibr_occl":
        ol, orr = orc.dibr_occl(a["disp_l"], a["disp_r"])
        return {"occl_l": ol, "occl_r": orr}
    if stage == "dibr_occl_to_mask":
        ml, mr = orc.dibr_occl_to_mask(a["occl_l"], a["occl_r"])
        return {"mask_l": ml, "mask_r": mr}
    if stage == "dibr_dbm":
        return {"view": orc.dibr_dbm(a["img_l"], a["img_r"], a["disp_l"], a["disp_r"], a["mask_l"], a["mask_r"], p["shift"], 7, 10.0)}
    if stage == "mux_multiview":
        variant = 2 if p["Hout"] % len(a["views"]) == 0 else 1
        return {"out": orc.mux_multiview(list(a["views"]), p["angle"], p["Hout"], p["Wout"], variant)}
    if stage == "tx_scale":
        return {"out": orc.tx_scale_bilinear(a["img"], p["Hout"], p["Wout"])}
    raise AssertionError(stage)


def run_hip(stm, stage, p, a, quirks=True):
    """The HIP library through its host-flavour API on the same arrays."""
    from stm_amd import host_api as api
    if stage == "ci_adcensus":
        stm.lib().stm_set_ref_quirks(1 if quirks else 0)
        try:
            cl, cr = api.ci_adcensus(a["img_l"], a["img_r"], p["ad_coeff"], p["census_coeff"], p["D"], p["zd"])
        finally:
            stm.lib().stm_set_ref_quirks(0)
        return {"cost_l": cl, "cost_r": cr}
    if stage == "ca_cross":
        cross, acost = api.ca_cross(a["img"], a["cost"], p["ucd"], p["lcd"], p["usd"], p["lsd"])
        return {"cross": cross, "acost": acost}
    if stage == "dc_wta":
        return {"disp": api.dc_wta(a["cost"], p["zd"])}
    if stage == "dr_dcc":
        ol, orr = api.dr_dcc(a["disp_l"], a["disp_r"])
        return {"outliers_l": ol, "outliers_r": orr}
    if stage == "filter_bilateral_1":
        return {"img": api.filter_bilateral_1(a["img"], p["radius"], p["sigma_color"], p["sigma_spatial"], p["D"])}
    if stage == "filter_gaussian_1":
        return {"img": api.filter_gaussian_1(a["img"], p["radius"], p["sigma"])}
    if stage == "filter_bleed_1":
        return {"img": api.filter_bleed_1(a["img"], p["radius"])}
    if stage == "dibr_occl":
        ol, orr = api.dibr_occl(a["disp_l"], a["disp_r"])
        return {"occl_l": ol, "occl_r": orr}
    if stage == "dibr_occl_to_mask":
        ml, mr = api.dibr_occl_to_mask(a["occl_l"], a["occl_r"])
        return {"mask_l": ml, "mask_r": mr}
    if stage == "dibr_dbm":
        return {"view": api.dibr_dbm(a["img_l"], a["img_r"], a["disp_l"], a["disp_r"], a["occl_l"], a["occl_r"], a["mask_l"],
                                     a["mask_r"], p["shift"])}
    if stage == "mux_multiview":
        return {"out": api.mux_multiview(list(a["views"]), p["angle"], p["Hout"], p["Wout"])}
    if stage == "tx_scale":
        return {"out": api.tx_scale(a["img"], p["Hout"], p["Wout"])}
    raise AssertionError(stage)


SAMPLE = 40000  # elements of a volume kept in a recorded fixture
WHOLE = 70000   # arrays up to this many elements are recorded whole


def views_of(name, out):
    """What of a stage's outputs is recorded and compared on the CPU: small arrays whole; of a volume a fixed seeded sample of
    SAMPLE elements plus the whole first plane (for cost init the d = 0 plane, where A-Q7 acts).  The same function is applied to the
    oracle's outputs before they are compared with a recorded fixture."""
    v = {}
    for k in sorted(out):
        arr = out[k]
        if arr.size <= WHOLE:
            v[k] = arr
            continue
        idx = np.random.RandomState(zlib.crc32((name + k).encode()) & 0x7FFFFFFF).choice(arr.size, SAMPLE, replace=False)
        v[k + "@sample"] = arr.reshape(-1)[np.sort(idx)]
        if arr.ndim == 3 and arr.shape[1] * arr.shape[2] <= WHOLE:
            v[k + "@d0"] = arr[0]
    return v


def same_with_nans(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return bool(a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


def max_abs_diff(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.size else 0.0


def check(stage, got, want, what):
    """Asserts the stage's rule key by key; `got` and `want` hold the same keys (whole outputs or views_of them).  Returns
    {key: max |got - want|} of the float keys, printed before asserting so a failing run still shows the figures."""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    figures = {}
    for k in sorted(got):
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        rule = RULES[stage][k.split("@")[0]]
        if g.dtype.kind == "f":
            fin = np.isfinite(g) & np.isfinite(w)
            figures[k] = max_abs_diff(g[fin], w[fin])
            print("%s %s %s: max |diff| = %.9g, differing = %d of %d" % (what, stage, k, figures[k], int((g != w).sum()), g.size))
        if rule == "exact":
            if g.dtype.kind == "f":
                assert np.array_equal(np.isfinite(g), np.isfinite(w)), "%s %s: non-finite values at different places" % (what, k)
                assert same_with_nans(g, w), "%s %s: %d of %d elements differ" % (what, k, int((g != w).sum()), g.size)
            else:
                assert np.array_equal(g, w), "%s %s: %d of %d elements differ" % (what, k, int((g != w).sum()), g.size)
        else:
            tol = TOL[stage]
            assert np.isfinite(g).all() and np.isfinite(w).all()
            bad = np.abs(g.astype(np.float64) - w.astype(np.float64)) > tol
            assert not bad.any(), "%s %s: %d elements differ by more than %g (max %g)" % (what, k, int(bad.sum()), tol, figures[k])
    return figures


def q7_columns(shape, side):
    """The elements of a cost volume where SURVEY A-Q7 predicts the reference's stray tile reads: d = 0, block column 0 for
    the left cost and block column 159 for the right cost of every 160-wide block."""
    m = np.zeros(shape, bool)
    m[0, :, (0 if side == "l" else 159)::160] = True
    return m


def _q7_mask(name, key, shape, side):
    full = q7_columns(shape, side)
    base = key.split("@")[0]
    return full if "@" not in key else views_of(name, {base: full})[key]


def check_q7(name, shape, got, clean, quirk, tol, what):
    """Cost init with quirks OFF: the reference (`got`) may differ from the clean oracle (`clean`) by more than the tolerance only
    in the columns A-Q7 predicts, nowhere else; and wherever the oracle's own quirk mode (`quirk`) departs from the clean mode by
    more than 3 * tol, the reference departs too (it lies within tol of the quirk mode).  All three are whole outputs or views_of
    them with the same keys."""
    for k in sorted(got):
        side = "l" if k.startswith("cost_l") else "r"
        g, c, q = (x[k].astype(np.float64) for x in (got, clean, quirk))
        bad = np.abs(g - c) > tol
        pred = _q7_mask(name, k, shape, side)
        strong = np.abs(q - c) > 3 * tol
        print("%s clean-mode %s: %d elements beyond tolerance, %d outside the A-Q7 columns; oracle quirk mode departs at %d" %
              (what, k, int(bad.sum()), int((bad & ~pred).sum()), int(strong.sum())))
        assert not (bad & ~pred).any(), "%s differs from the clean oracle outside the A-Q7 columns" % k
        assert not (strong & ~pred).any() and not (strong & ~bad).any(), "%s: a predicted stray read is not in the reference" % k


CHILD_SECONDS = 240


def reference_child(tmp_dir, stage, params, arrays, tag="call"):
    """One reference stage call in a child process (python -m oracle.pyref under `timeout`): the reference ends the process with
    exit(1) on a failed runtime call.  Returns (status, outputs or None, tail of the child's output)."""
    src, dst = os.path.join(str(tmp_dir), tag + "_in.npz"), os.path.join(str(tmp_dir), tag + "_out.npz")
    np.savez(src, stage=stage, params=json.dumps(params), **arrays)
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, "-m", "oracle.pyref", src, dst]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    tail = r.stdout.decode(errors="replace")[-4000:]
    if r.returncode != 0 or not os.path.exists(dst):
        return (r.returncode or 1), None, tail
    return 0, dict(np.load(dst)), tail
