"""What the shot-change detector buys the recursive states, measured on the CPU oracle and the numpy statements (no GPU): six frames
of the committed bud pair (tests/golden/bud_2 + bud_3), then six of the fish pair (fish_1 + fish_2), 640 x 384, D = 32, zero_disp 16
(the parameters of tools/align_effect.py).
  - Depth mode 2 at rate 0.1, budget [-4, 4], max_gain 4, clip 20: for each frame after the cut, the distance of the applied gain
    and convergence (the statement of tests/test_depth_ref.py on the oracle's maps) from the fresh fit on that frame, without the
    detector and with it (tests/test_cut_ref.py's statement at the default threshold and min_gap decides where `valid` is zeroed).
  - Alignment mode 2 at rate 0.1, radius 16, the second shot's right eye displaced by (2.2, -0.006, 0.01): likewise the largest
    difference, over the four corners of the eye, between the applied field and the fresh fit, in rows.
usage: python tools/cut_effect.py [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

P = dict(D=32, zd=16, ad=10.0, ce=30.0, ucd=6.0, lcd=20.0, usd=17, lsd=8, ts=20, th=0.4, N=8, angle=18.43)
SHOTS = [("bud", ("bud_2.bmp", "bud_3.bmp")), ("fish", ("fish_1.bmp", "fish_2.bmp"))]
PER_SHOT = 6
RATE = 0.1
BUDGET = (-4.0, 4.0, 4.0, 20)
FIELD = (2.2, -0.006, 0.01)
RADIUS = 16


def corner_distance(H, W, f, g):
    """the largest |dy_f - dy_g| over the four corners of an eye, dy = a + b u + c v from the centre"""
    worst = 0.0
    for u in (-(W - 1) / 2.0, (W - 1) / 2.0):
        for v in (-(H - 1) / 2.0, (H - 1) / 2.0):
            worst = max(worst, abs((f[0] - g[0]) + (f[1] - g[1]) * u + (f[2] - g[2]) * v))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import stm_amd
    from stm_amd import video
    from oracle import pyoracle as orc
    from test_align_ref import displace, measure_ref
    from test_cut_ref import detect_ref
    from test_depth_ref import depth_fit_ref
    orc.build()
    thresh, min_gap = video.CUT_DEFAULT

    pairs, maps = [], []
    for k, (name, files) in enumerate(SHOTS):
        L, R = (stm_amd.bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", f)) for f in files)
        if k == 1:
            R = np.ascontiguousarray(displace(R, *FIELD))
        H, W, _ = L.shape
        sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
        o = orc.adcensus_stm(sbs, H, W, P["N"], P["angle"], P["D"], P["zd"], P["ad"], P["ce"], P["ucd"], P["lcd"], P["usd"], P["lsd"], P["ts"],
                             P["th"])
        pairs.append((L, R))
        maps.append((o["disp_l"], o["disp_r"]))
    order = [0] * PER_SHOT + [1] * PER_SHOT
    fresh_depth = [depth_fit_ref(*maps[s], *BUDGET, 1.0, (0, 0, 0, 0)) for s in (0, 1)]
    fresh_align = [measure_ref(*pairs[s], RADIUS)[2] for s in (0, 1)]

    res = {"params": P, "shots": [s[0] for s in SHOTS], "frames_per_shot": PER_SHOT, "rate": RATE, "depth_budget": list(BUDGET),
           "align_field_of_second_shot": list(FIELD), "align_radius": RADIUS, "thresh_permille": thresh, "min_gap": min_gap,
           "fresh_depth": [[float(v) for v in f[1:3]] for f in fresh_depth], "fresh_align": [[float(v) for v in f[1:]] for f in fresh_align],
           "frames": []}
    H, W = pairs[0][0].shape[:2]
    runs = {}
    for detector in (False, True):
        depth, align, cut = np.zeros(4, np.float32), np.zeros(4, np.float32), None
        rows = []
        for k, s in enumerate(order):
            flag = score = 0
            if detector:
                cut = detect_ref(pairs[s][0], cut, thresh, min_gap)
                flag, score = int(cut[1]), int(cut[3])
                if flag:
                    depth[0] = 0
                    align[0] = 0
            align = measure_ref(*pairs[s], RADIUS, align, RATE)[2]
            depth = depth_fit_ref(*maps[s], *BUDGET, RATE, depth)
            rows.append({"frame": k, "shot": SHOTS[s][0], "cut": flag, "score": score,
                         "gain_distance": abs(float(depth[1]) - float(fresh_depth[s][1])),
                         "conv_distance": abs(float(depth[2]) - float(fresh_depth[s][2])),
                         "align_corner_distance_rows": corner_distance(H, W, [float(v) for v in align[1:]], [float(v) for v in fresh_align[s][1:]])})
        runs[detector] = rows
    for k in range(PER_SHOT, 2 * PER_SHOT):
        row = {"frame": k, "cut_flag_with_detector": runs[True][k]["cut"], "score": runs[True][k]["score"]}
        for key in ("gain_distance", "conv_distance", "align_corner_distance_rows"):
            row[key + "_without"] = runs[False][k][key]
            row[key + "_with"] = runs[True][k][key]
        print(json.dumps(row), flush=True)
        res["frames"].append(row)
    res["cut_flags_with_detector"] = [r["cut"] for r in runs[True]]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
