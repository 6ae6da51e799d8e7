"""ctypes/numpy loader of oracle/_ref/libstm_ref_hip.so: the reference project's own kernels, compiled for gfx950 by
oracle/build_ref.py.  TEST INFRASTRUCTURE ONLY (tests/test_gpu_reference.py, tests/golden/make_golden_ref.py); the
product package, smoke() and bench.py never load it.

Only the reference's HOST-flavour functions are called, by mangled name, with numpy arrays: they allocate, copy and
launch by themselves.  After every call `_sync()` calls hipDeviceSynchronize and hipGetLastError and raises on an
error, because the reference checks no launch status (SURVEY A-L1) and a launch that silently failed would hand back
stale memory.  The reference ends the process with exit(1) on a failed runtime call, so this module is meant to be
used from a CHILD process:

    python -m oracle.pyref IN.npz OUT.npz

IN.npz holds the arrays of one stage call plus `stage` (name) and `params` (JSON); OUT.npz receives the outputs.

`admit(stage, **shape)` is the envelope of SURVEY Appendix A (L1-L9): it raises before anything is launched on a
shape for which the reference's index arithmetic leaves its tiles or buffers.  tests/test_gpu_reference.py says, stage
by stage, why the admitted shapes stay in bounds, and which stages are left out because that cannot be shown.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libstm_ref_hip.so")
_LIB = None

u8p = C.POINTER(C.c_uint8)
f32p = C.POINTER(C.c_float)
LDS_LIMIT = 64 * 1024  # default dynamic LDS limit of a launch on gfx950

_I, _F = C.c_int, C.c_float
_PROTOS = {
    "ci_adcensus": ("_Z11ci_adcensusPhS_PPfS1_ffiiiii", [u8p, u8p, C.POINTER(f32p), C.POINTER(f32p), _F, _F, _I, _I, _I, _I, _I]),
    "ca_cross": ("_Z8ca_crossPhPS_PPfS2_ffiiiiii", [u8p, C.POINTER(u8p), C.POINTER(f32p), C.POINTER(f32p), _F, _F, _I, _I, _I, _I, _I, _I]),
    "dc_wta": ("_Z6dc_wtaPPfS_iiii", [C.POINTER(f32p), f32p, _I, _I, _I, _I]),
    "dr_dcc": ("_Z6dr_dccPhS_PfS0_ii", [u8p, u8p, f32p, f32p, _I, _I]),
    "filter_bilateral_1": ("_Z18filter_bilateral_1Pfiffiii", [f32p, _I, _F, _F, _I, _I, _I]),
    "filter_gaussian_1": ("_Z17filter_gaussian_1Pfifii", [f32p, _I, _F, _I, _I]),
    "filter_bleed_1": ("_Z14filter_bleed_1Phiii", [u8p, _I, _I, _I]),
    "dibr_occl": ("_Z9dibr_occlPhS_PfS0_ii", [u8p, u8p, f32p, f32p, _I, _I]),
    "dibr_occl_to_mask": ("_Z17dibr_occl_to_maskPfS_PhS0_ii", [f32p, f32p, u8p, u8p, _I, _I]),
    "dibr_dbm": ("_Z8dibr_dbmPhS_S_PfS0_S_S_S0_S0_fiii", [u8p, u8p, u8p, f32p, f32p, u8p, u8p, f32p, f32p, _F, _I, _I, _I]),
    "mux_multiview": ("_Z13mux_multiviewPPhS_ifiiiii", [C.POINTER(u8p), u8p, _I, _F, _I, _I, _I, _I, _I]),
    "tx_scale": ("_Z10d_tx_scalePhS_iiiii", [u8p, u8p, _I, _I, _I, _I, _I]),  # host pointers despite its d_ name
}


def available():
    return os.path.exists(LIB_PATH)


def lib():
    global _LIB
    if _LIB is None:
        if not available():
            raise RuntimeError("oracle/_ref/libstm_ref_hip.so is missing: build() makes it where the reference tree exists "
                               "(oracle/build_ref.py) and it travels with the tree from there")
        _LIB = C.CDLL(LIB_PATH, mode=getattr(os, "RTLD_LOCAL", 0) | getattr(os, "RTLD_NOW", 2))
        for name, (sym, args) in _PROTOS.items():
            fn = getattr(_LIB, sym)
            fn.argtypes, fn.restype = args, None
        _LIB.hipDeviceSynchronize.restype = C.c_int
        _LIB.hipGetLastError.restype = C.c_int
    return _LIB


def _fn(name):
    return getattr(lib(), _PROTOS[name][0])


def _sync(what):
    a = lib().hipDeviceSynchronize()
    b = lib().hipGetLastError()
    if a != 0 or b != 0:
        raise RuntimeError("%s: hipDeviceSynchronize -> %d, hipGetLastError -> %d" % (what, a, b))


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a, a.ctypes.data_as(u8p)


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(f32p)


def _planes_f32(vol):
    return (f32p * vol.shape[0])(*[vol[d].ctypes.data_as(f32p) for d in range(vol.shape[0])])


def _planes_u8(vol):
    return (u8p * vol.shape[0])(*[vol[k].ctypes.data_as(u8p) for k in range(vol.shape[0])])


def admit(stage, H, W, D=1, zd=0, usd=1, radius=0, Hout=None, Wout=None, N=8):
    """The reference's launch envelope.  Raises AssertionError outside it."""
    assert stage in _PROTOS, "%s is not admitted (see tests/test_gpu_reference.py for the stages left out)" % stage
    assert 0 < W <= 1024 and W % 2 == 0 and H > 0 and H % 2 == 0, "A-L1, A-L2"
    assert 1 <= D <= 65 and 0 <= zd < D, "A-L7"
    lds = 0
    if stage == "ci_adcensus":
        assert W % 160 == 0, "A-L4"
        pad = (D - zd) if (D - zd) > zd else zd - 1
        lds = max((160 + 2 * pad) * 3 * 2, (160 + D - 1) * 8 * 2)
    elif stage == "ca_cross":
        assert W % 32 == 0 and H % 32 == 0 and H <= 2048, "A-L2, A-L3"
        assert 1 <= usd <= 255
        lds = (3 * max(W, H) + 1) * 4
    elif stage == "filter_bilateral_1":
        assert H % 30 == 0 and W % 32 == 0, "A-L6"
        assert 1 <= radius <= 15
        lds = ((30 + 2 * radius) * (32 + 2 * radius) + (2 * radius + 1) ** 2 + D) * 4
    elif stage in ("filter_gaussian_1", "dibr_dbm"):
        radius = radius if stage == "filter_gaussian_1" else 7
        assert H % 32 == 0 and W % 32 == 0, "A-L5"
        assert 1 <= radius <= 15
        lds = ((32 + 2 * radius) ** 2 + (2 * radius + 1) ** 2) * 4
    elif stage == "filter_bleed_1":
        assert 1 <= radius < min(H, W)
    elif stage == "tx_scale":
        assert 0 < Hout <= 4096 and 0 < Wout <= 4096
    elif stage == "mux_multiview":
        assert Hout > 0 and Wout > 0 and 2 <= N <= 16
        if Hout % N == 0:  # the strided kernel: a ragged width writes one pixel past a row
            assert Wout % N == 0 and Wout // N <= 1024
    assert lds <= LDS_LIMIT, "A-L9: dynamic LDS request %d B" % lds
    return True


def ci_adcensus(img_l, img_r, ad_coeff, census_coeff, D, zd):
    H, W, E = img_l.shape
    admit("ci_adcensus", H, W, D, zd)
    assert E == 3 and img_r.shape == img_l.shape
    img_l, pl = _u8(img_l)
    img_r, pr = _u8(img_r)
    cl = np.zeros((D, H, W), np.float32)
    cr = np.zeros((D, H, W), np.float32)
    _fn("ci_adcensus")(pl, pr, _planes_f32(cl), _planes_f32(cr), ad_coeff, census_coeff, D, zd, H, W, E)
    _sync("ci_adcensus")
    return cl, cr


def ca_cross(img, cost, ucd, lcd, usd, lsd):
    H, W, E = img.shape
    D = cost.shape[0]
    admit("ca_cross", H, W, D, 0, usd)
    assert E == 3 and cost.shape == (D, H, W)
    img, pi = _u8(img)
    cost = np.array(cost, dtype=np.float32, order="C", copy=True)
    cross = np.zeros((4, H, W), np.uint8)
    acost = np.zeros_like(cost)
    _fn("ca_cross")(pi, _planes_u8(cross), _planes_f32(cost), _planes_f32(acost), ucd, lcd, usd, lsd, D, H, W, E)
    _sync("ca_cross")
    return cross, acost


def dc_wta(cost, zd):
    D, H, W = cost.shape
    admit("dc_wta", H, W, D, zd)
    cost, _ = _f32(cost)
    disp = np.zeros((H, W), np.float32)
    _fn("dc_wta")(_planes_f32(cost), disp.ctypes.data_as(f32p), D, zd, H, W)
    _sync("dc_wta")
    return disp


def dr_dcc(disp_l, disp_r):
    H, W = disp_l.shape
    admit("dr_dcc", H, W)
    disp_l, pl = _f32(disp_l)
    disp_r, pr = _f32(disp_r)
    ol = np.zeros((H, W), np.uint8)
    orr = np.zeros((H, W), np.uint8)
    _fn("dr_dcc")(ol.ctypes.data_as(u8p), orr.ctypes.data_as(u8p), pl, pr, H, W)
    _sync("dr_dcc")
    return ol, orr


def filter_bilateral_1(img, radius, sigma_color, sigma_spatial, D):
    H, W = img.shape
    admit("filter_bilateral_1", H, W, D, 0, radius=radius)
    img = np.array(img, dtype=np.float32, order="C", copy=True)
    # the colour table has D entries and is indexed by (int)|a - b| with no clamp
    assert float(img.max()) - float(img.min()) < D and np.isfinite(img).all(), "A-Q18: value range must stay below num_disp"
    _fn("filter_bilateral_1")(img.ctypes.data_as(f32p), radius, sigma_color, sigma_spatial, H, W, D)
    _sync("filter_bilateral_1")
    return img


def filter_gaussian_1(img, radius, sigma):
    H, W = img.shape
    admit("filter_gaussian_1", H, W, radius=radius)
    img = np.array(img, dtype=np.float32, order="C", copy=True)
    _fn("filter_gaussian_1")(img.ctypes.data_as(f32p), radius, sigma, H, W)
    _sync("filter_gaussian_1")
    return img


def filter_bleed_1(img, radius):
    H, W = img.shape
    admit("filter_bleed_1", H, W, radius=radius)
    img = np.array(img, dtype=np.uint8, order="C", copy=True)
    _fn("filter_bleed_1")(img.ctypes.data_as(u8p), radius, H, W)
    _sync("filter_bleed_1")
    return img


def dibr_occl(disp_l, disp_r):
    H, W = disp_l.shape
    admit("dibr_occl", H, W)
    disp_l, pl = _f32(disp_l)
    disp_r, pr = _f32(disp_r)
    ol = np.zeros((H, W), np.uint8)
    orr = np.zeros((H, W), np.uint8)
    _fn("dibr_occl")(ol.ctypes.data_as(u8p), orr.ctypes.data_as(u8p), pl, pr, H, W)
    _sync("dibr_occl")
    return ol, orr


def dibr_occl_to_mask(occl_l, occl_r):
    H, W = occl_l.shape
    admit("dibr_occl_to_mask", H, W)
    occl_l, pl = _u8(occl_l)
    occl_r, pr = _u8(occl_r)
    ml = np.zeros((H, W), np.float32)
    mr = np.zeros((H, W), np.float32)
    _fn("dibr_occl_to_mask")(ml.ctypes.data_as(f32p), mr.ctypes.data_as(f32p), pl, pr, H, W)
    _sync("dibr_occl_to_mask")
    return ml, mr


def dibr_dbm(img_l, img_r, disp_l, disp_r, occl_l, occl_r, mask_l, mask_r, shift):
    H, W, E = img_l.shape
    admit("dibr_dbm", H, W)
    assert E == 3 and np.isfinite(disp_l).all() and np.isfinite(disp_r).all()
    img_l, pil = _u8(img_l)
    img_r, pir = _u8(img_r)
    disp_l, pdl = _f32(disp_l)
    disp_r, pdr = _f32(disp_r)
    occl_l, pol = _u8(occl_l)
    occl_r, por = _u8(occl_r)
    mask_l, pml = _f32(mask_l)
    mask_r, pmr = _f32(mask_r)
    out = np.zeros((H, W, E), np.uint8)
    _fn("dibr_dbm")(out.ctypes.data_as(u8p), pil, pir, pdl, pdr, pol, por, pml, pmr, shift, H, W, E)
    _sync("dibr_dbm")
    return out


def mux_multiview(views, angle, Hout, Wout):
    views = [np.ascontiguousarray(v, dtype=np.uint8) for v in views]
    N = len(views)
    H, W, E = views[0].shape
    admit("mux_multiview", H, W, Hout=Hout, Wout=Wout, N=N)
    assert E == 3 and all(v.shape == (H, W, E) for v in views) and abs(np.tan(np.deg2rad(angle))) > 1e-6, "A-Q24"
    tab = (u8p * N)(*[v.ctypes.data_as(u8p) for v in views])
    out = np.zeros((Hout, Wout, E), np.uint8)
    _fn("mux_multiview")(tab, out.ctypes.data_as(u8p), N, angle, H, W, Hout, Wout, E)
    _sync("mux_multiview")
    return out


def tx_scale(img, Hout, Wout):
    H, W, E = img.shape
    admit("tx_scale", H, W, Hout=Hout, Wout=Wout)
    assert E == 3
    img, pi = _u8(img)
    out = np.zeros((Hout, Wout, E), np.uint8)
    _fn("tx_scale")(pi, out.ctypes.data_as(u8p), H, W, Hout, Wout, E)
    _sync("tx_scale")
    return out


def run_call(stage, p, a):
    """One stage call described by data: `p` parameters, `a` input arrays.  Returns {name: array}."""
    if stage == "ci_adcensus":
        cl, cr = ci_adcensus(a["img_l"], a["img_r"], p["ad_coeff"], p["census_coeff"], p["D"], p["zd"])
        return {"cost_l": cl, "cost_r": cr}
    if stage == "ca_cross":
        cross, acost = ca_cross(a["img"], a["cost"], p["ucd"], p["lcd"], p["usd"], p["lsd"])
        return {"cross": cross, "acost": acost}
    if stage == "dc_wta":
        return {"disp": dc_wta(a["cost"], p["zd"])}
    if stage == "dr_dcc":
        ol, orr = dr_dcc(a["disp_l"], a["disp_r"])
        return {"outliers_l": ol, "outliers_r": orr}
    if stage == "filter_bilateral_1":
        return {"img": filter_bilateral_1(a["img"], p["radius"], p["sigma_color"], p["sigma_spatial"], p["D"])}
    if stage == "filter_gaussian_1":
        return {"img": filter_gaussian_1(a["img"], p["radius"], p["sigma"])}
    if stage == "filter_bleed_1":
        return {"img": filter_bleed_1(a["img"], p["radius"])}
    if stage == "dibr_occl":
        ol, orr = dibr_occl(a["disp_l"], a["disp_r"])
        return {"occl_l": ol, "occl_r": orr}
    if stage == "dibr_occl_to_mask":
        ml, mr = dibr_occl_to_mask(a["occl_l"], a["occl_r"])
        return {"mask_l": ml, "mask_r": mr}
    if stage == "dibr_dbm":
        return {"view": dibr_dbm(a["img_l"], a["img_r"], a["disp_l"], a["disp_r"], a["occl_l"], a["occl_r"], a["mask_l"],
                                 a["mask_r"], p["shift"])}
    if stage == "mux_multiview":
        return {"out": mux_multiview(list(a["views"]), p["angle"], p["Hout"], p["Wout"])}
    if stage == "tx_scale":
        return {"out": tx_scale(a["img"], p["Hout"], p["Wout"])}
    raise AssertionError("stage %s is not admitted" % stage)


def main(argv):
    src, dst = argv
    z = np.load(src)
    stage = str(z["stage"])
    params = json.loads(str(z["params"]))
    arrays = {k: z[k] for k in z.files if k not in ("stage", "params")}
    # the reference prints its kernel timings to stdout; keep them out of the caller's way
    out = run_call(stage, params, arrays)
    sys.stdout.flush()
    np.savez(dst, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
