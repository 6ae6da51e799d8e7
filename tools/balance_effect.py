"""What the colour balance between the eyes buys the matcher, measured on the CPU oracle (no GPU): both committed pairs
(tests/golden/bud_2 + bud_3, fish_1 + fish_2, 640 x 384, D = 32, zero_disp 16, the parameters of tools/align_effect.py), the right eye
distorted per channel by floor(255 (x/255)^gamma * gain + offset + 0.5).  For each: the share of pixels whose final left disparity
(the oracle's adcensus_stm) differs by more than 1 from the undistorted pair's -- without the balance, and with mode 2 as the numpy
statement of tests/test_balance_ref.py computes it (max_shift 64, every frame on its own) -- and the mean absolute difference of the
right eye from the undistorted one before and after.
usage: python tools/balance_effect.py [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

P = dict(D=32, zd=16, ad=10.0, ce=30.0, ucd=6.0, lcd=20.0, usd=17, lsd=8, ts=20, th=0.4, N=8, angle=18.43)
PAIRS = {"bud": ("bud_2.bmp", "bud_3.bmp"), "fish": ("fish_1.bmp", "fish_2.bmp")}
SETTINGS = [((0.85, 0.85, 0.85), (0, 0, 0), (1, 1, 1)),
            ((0.9, 1.0, 1.1), (6, 0, -8), (1, 1, 1)),
            ((0.8, 0.95, 0.9), (10, -5, 4), (0.85, 1.1, 1.2))]
MAX_SHIFT = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import stm_amd
    from oracle import pyoracle as orc
    from test_balance_ref import apply_ref, distort, fit_ref, lut_ref
    orc.build()

    def disp_l(L, R):
        H, W, _ = L.shape
        sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
        return orc.adcensus_stm(sbs, H, W, P["N"], P["angle"], P["D"], P["zd"], P["ad"], P["ce"], P["ucd"], P["lcd"], P["usd"], P["lsd"],
                                P["ts"], P["th"])["disp_l"]

    res = {"params": P, "max_shift": MAX_SHIFT, "threshold": 1.0, "cases": []}
    for name, files in PAIRS.items():
        L, R = (stm_amd.bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", f)) for f in files)
        base = disp_l(L, R)
        for gain, offset, gamma in SETTINGS:
            bad = distort(R, gain, offset, gamma)
            _, state = fit_ref(L, bad, MAX_SHIFT)
            matched = np.ascontiguousarray(apply_ref(bad, lut_ref(state)))
            off = float((np.abs(disp_l(L, bad) - base) > 1.0).mean())
            on = float((np.abs(disp_l(L, matched) - base) > 1.0).mean())
            case = {"pair": name, "gain": list(gain), "offset": list(offset), "gamma": list(gamma), "share_off": off, "share_mode_2": on,
                    "mad_distorted": float(np.abs(bad.astype(np.int32) - R).mean()), "mad_matched": float(np.abs(matched.astype(np.int32) - R).mean())}
            print(json.dumps(case), flush=True)
            res["cases"].append(case)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
