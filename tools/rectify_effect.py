"""What the rectification buys, measured on the CPU oracle (no GPU): both committed pairs (tests/golden/bud_2 + bud_3, fish_1 +
fish_2, 640 x 384, D = 32, zero_disp 16, the parameters of tests/golden/make_golden_c1.py).  The right eye is seen through a camera
rolled by 1 degree, with a focal ratio fy / fx of 1.02 and k1 = -0.05: the distorted eye is the clean one sampled bilinearly in
float64 at the inverse of the camera model (the model's forward map inverted by fixed-point iteration), so that rectifying it with
the camera's record brings the clean eye back up to two resamplings.  For each pair: the share of pixels whose final left disparity
(the oracle's adcensus_stm) differs by more than 1 from the undistorted pair's -- without rectification, with rectification (the numpy
statement of tests/test_rectify_ref.py, border 1, the left eye through the identity), and with the automatic vertical alignment
alone (tests/test_align_ref.py, radius 16).
usage: python tools/rectify_effect.py [--out FILE.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

P = dict(D=32, zd=16, ad=10.0, ce=30.0, ucd=6.0, lcd=20.0, usd=17, lsd=8, ts=20, th=0.4, N=8, angle=18.43)
PAIRS = {"bud": ("bud_2.bmp", "bud_3.bmp"), "fish": ("fish_1.bmp", "fish_2.bmp")}
ROLL_DEG, FOCAL_RATIO, K1 = 1.0, 1.02, -0.05


def model(rec, x, y):
    """the record's forward map in float64: rectified pixel (x, y) -> source position (u, v)"""
    c = rec.astype(np.float64)
    X, Y, Wd = c[0] * x + c[1] * y + c[2], c[3] * x + c[4] * y + c[5], c[6] * x + c[7] * y + c[8]
    xn, yn = X / Wd, Y / Wd
    r2 = xn * xn + yn * yn
    rad = 1.0 + r2 * (c[13] + r2 * (c[14] + r2 * c[17]))
    xd = xn * rad + 2.0 * c[15] * xn * yn + c[16] * (r2 + 2.0 * xn * xn)
    yd = yn * rad + c[15] * (r2 + 2.0 * yn * yn) + 2.0 * c[16] * xn * yn
    return c[9] * xd + c[11], c[10] * yd + c[12]


def distort(img, rec, iterations=40):
    """the eye the camera of `rec` sees where `img` is the rectified one: pixel (u, v) of the result is img sampled at the (x, y)
    with model(x, y) = (u, v), found by the fixed-point iteration (x, y) <- (x, y) + ((u, v) - model(x, y)); float64 bilinear
    sampling, coordinates clamped.  Returns the image and the largest residual of the iteration in pixels."""
    H, W = img.shape[:2]
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    x, y = u.copy(), v.copy()
    for _ in range(iterations):
        mu, mv = model(rec, x, y)
        x, y = x + (u - mu), y + (v - mv)
    mu, mv = model(rec, x, y)
    resid = float(max(np.abs(mu - u).max(), np.abs(mv - v).max()))
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    src = img.astype(np.float64)
    tap = lambda ty, tx: src[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)]
    top = (1.0 - fx) * tap(yi, xi) + fx * tap(yi, xi + 1)
    bot = (1.0 - fx) * tap(yi + 1, xi) + fx * tap(yi + 1, xi + 1)
    return np.clip(np.floor((1.0 - fy) * top + fy * bot + 0.5), 0, 255).astype(np.uint8), resid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import stm_amd
    from stm_amd import rectify
    from oracle import pyoracle as orc
    from test_align_ref import align_rows_ref, measure_ref
    from test_rectify_ref import rectify_ref
    orc.build()

    def disp_l(L, R):
        H, W, _ = L.shape
        sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
        return orc.adcensus_stm(sbs, H, W, P["N"], P["angle"], P["D"], P["zd"], P["ad"], P["ce"], P["ucd"], P["lcd"], P["usd"], P["lsd"],
                                P["ts"], P["th"])["disp_l"]

    res = {"params": P, "roll_deg": ROLL_DEG, "focal_ratio": FOCAL_RATIO, "k1": K1, "border": 1, "threshold": 1.0, "cases": []}
    for name, files in PAIRS.items():
        L, R = (stm_amd.bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", f)) for f in files)
        H, W, _ = L.shape
        a = math.radians(ROLL_DEG)
        newK = np.array([[1.0 * W, 0.0, (W - 1) / 2.0], [0.0, 1.0 * W, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
        K = newK.copy()
        K[1, 1] *= FOCAL_RATIO
        roll = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        rec = rectify.record(K, [K1], roll, newK)
        seen, resid = distort(R, rec)
        base = disp_l(L, R)
        share = lambda right: float((np.abs(disp_l(L, np.ascontiguousarray(right)) - base) > 1.0).mean())
        _, _, state, nvalid = measure_ref(L, seen, 16)
        fit = [float(v) for v in state[1:]]
        top, bottom, left, right = rectify.inner_rect(rec, H, W)
        case = {"pair": name, "inverse_residual_px": resid, "share_without": share(seen),
                "share_rectified": share(rectify_ref(seen, rec, 1)), "share_align_auto_alone": share(align_rows_ref(seen, *fit)),
                "align_fit": fit, "align_valid_blocks": nvalid, "inner_rect": [top, bottom, left, right]}
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
