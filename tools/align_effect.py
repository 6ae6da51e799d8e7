"""What the vertical alignment buys, measured on the CPU oracle (no GPU): both committed pairs (tests/golden/bud_2 + bud_3,
fish_1 + fish_2, 640 x 384, D = 32, zero_disp 16, the parameters of tests/golden/make_golden_c1.py), the right eye displaced by
(3.3, 0, 0) and by (2.2, -0.006, 0.01) with float bilinear resampling.  For each: the share of pixels whose final left disparity
(the oracle's adcensus_stm) differs by more than 1 from the undisplaced pair's -- without alignment, and with mode 2 as the numpy
statement of tests/test_align_ref.py computes it (measure at radius 16, every frame on its own, then apply).
usage: python tools/align_effect.py [--out FILE.json]"""
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
FIELDS = [(3.3, 0.0, 0.0), (2.2, -0.006, 0.01)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import stm_amd
    from oracle import pyoracle as orc
    from test_align_ref import align_rows_ref, displace, measure_ref
    orc.build()

    def disp_l(L, R):
        H, W, _ = L.shape
        sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
        return orc.adcensus_stm(sbs, H, W, P["N"], P["angle"], P["D"], P["zd"], P["ad"], P["ce"], P["ucd"], P["lcd"], P["usd"], P["lsd"],
                                P["ts"], P["th"])["disp_l"]

    res = {"params": P, "radius": 16, "threshold": 1.0, "cases": []}
    for name, files in PAIRS.items():
        L, R = (stm_amd.bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", f)) for f in files)
        base = disp_l(L, R)
        for field in FIELDS:
            moved = displace(R, *field)
            _, _, state, nvalid = measure_ref(L, moved, 16)
            fit = [float(v) for v in state[1:]]
            off = float((np.abs(disp_l(L, moved) - base) > 1.0).mean())
            on = float((np.abs(disp_l(L, np.ascontiguousarray(align_rows_ref(moved, *fit))) - base) > 1.0).mean())
            case = {"pair": name, "field": list(field), "fit": fit, "valid_blocks": nvalid, "share_off": off, "share_mode_2": on}
            print(json.dumps(case), flush=True)
            res["cases"].append(case)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
