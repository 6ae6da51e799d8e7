"""What the overlay's automatic placement buys, measured on the CPU oracle's maps and the numpy statement (no GPU): the committed bud
pair (tests/golden/bud_2 + bud_3) and the fish pair (fish_1 + fish_2), 640 x 384, D = 32, zero_disp 16 (the parameters of
tools/cut_effect.py), views of the maps' size, no depth budget.

The overlay is a full-width subtitle strip of 24 rows whose text -- an opaque box a third of the width -- sits over the nearest
third-width window of the bud pair's maps (the least mean of min(disp_l, disp_r) over all window positions): a subtitle over a near
object.  The metric is the share of the overlay's opaque pixels whose displayed scene disparity, min(disp_l, disp_r) at that pixel,
is nearer (smaller) than the overlay's: the depth conflicts.
  - a fixed disparity 0, per shot;
  - the placement at the tool's defaults (near 20, margin 1, pad 8, rates 1 and 0.1; limits -40 .. 10), a fresh fit per shot;
  - a three-shot sequence bud x 4, fish x 4, bud x 4 at those defaults (rate_far 0.1), without and with the shot-change detector
    (tests/test_cut_ref.py's statement at the default threshold and min_gap sets the cut flag the fit reads).
usage: python tools/overlay_fit_effect.py [--out FILE.json]"""
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
ORDER = [0] * 4 + [1] * 4 + [0] * 4
LIMITS = (-40.0, 10.0)
ROWS = 24


def nearest_window(near, rows, cols):
    """(y, x) of the rows x cols window with the least sum of `near`"""
    c = np.pad(np.cumsum(np.cumsum(near.astype(np.float64), axis=0), axis=1), ((1, 0), (1, 0)))
    s = c[rows:, cols:] - c[:-rows, cols:] - c[rows:, :-cols] + c[:-rows, :-cols]
    y, x = np.unravel_index(int(np.argmin(s)), s.shape)
    return int(y), int(x)


def conflicts(near, ov, x0, y0, disparity):
    """the share of the overlay's pixels with alpha != 0 under which the scene is displayed nearer than `disparity`"""
    on = ov[..., 3] != 0
    under = near[y0:y0 + ov.shape[0], x0:x0 + ov.shape[1]]
    return float((under[on] < disparity).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import stm_amd
    from stm_amd import device_api as dev, video
    from oracle import pyoracle as orc
    from test_cut_ref import detect_ref
    from test_overlay_fit_ref import overlay_fit_ref, state_disparity_ref
    orc.build()
    thresh, min_gap = video.CUT_DEFAULT
    near_permille, margin, pad, rate_near, rate_far = dev.OVERLAY_AUTO_DEFAULTS
    kw = dict(near_permille=near_permille, margin=margin, pad=pad, limit_lo=LIMITS[0], limit_hi=LIMITS[1], rate_near=rate_near, rate_far=rate_far)

    lefts, maps = [], []
    for name, files in SHOTS:
        L, R = (stm_amd.bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", f)) for f in files)
        H, W, _ = L.shape
        sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
        o = orc.adcensus_stm(sbs, H, W, P["N"], P["angle"], P["D"], P["zd"], P["ad"], P["ce"], P["ucd"], P["lcd"], P["usd"], P["lsd"], P["ts"], P["th"])
        lefts.append(L)
        maps.append((o["disp_l"], o["disp_r"]))
    H, W = maps[0][0].shape
    nears = [np.minimum(dl, dr) for dl, dr in maps]
    y0, q0 = nearest_window(nears[0], ROWS, W // 3)
    ov = np.zeros((ROWS, W, 4), np.uint8)
    ov[:, q0:q0 + W // 3] = 255

    res = {"params": P, "shots": [s[0] for s in SHOTS], "limits": list(LIMITS), "placement": kw, "overlay": {"rows": ROWS, "cols": W, "y0": y0,
           "text_cols": [q0, q0 + W // 3 - 1]}, "thresh_permille": thresh, "min_gap": min_gap}
    res["fixed_disparity_0"] = {SHOTS[s][0]: conflicts(nears[s], ov, 0, y0, 0.0) for s in (0, 1)}
    fresh = [overlay_fit_ref(*maps[s], ov, 0, y0, H, W, **kw) for s in (0, 1)]
    res["fresh_fit"] = {SHOTS[s][0]: {"disparity": state_disparity_ref(fresh[s], *LIMITS), "nearest": float(fresh[s][2]),
                                      "conflicts": conflicts(nears[s], ov, 0, y0, state_disparity_ref(fresh[s], *LIMITS))} for s in (0, 1)}
    res["sequence"] = {}
    for detector in (False, True):
        state, cut, rows = np.zeros(4, np.float32), None, []
        for k, s in enumerate(ORDER):
            flag = 0
            if detector:
                cut = detect_ref(lefts[s], cut, thresh, min_gap)
                flag = int(cut[1])
            state = overlay_fit_ref(*maps[s], ov, 0, y0, H, W, state=state, cut_flag=flag, **kw)
            d = state_disparity_ref(state, *LIMITS)
            rows.append({"frame": k, "shot": SHOTS[s][0], "cut": flag, "disparity": d, "fresh": state_disparity_ref(fresh[s], *LIMITS),
                         "conflicts": conflicts(nears[s], ov, 0, y0, d)})
            print(json.dumps(dict(rows[-1], detector=detector)), flush=True)
        res["sequence"]["with_detector" if detector else "without_detector"] = rows
    print(json.dumps({k: res[k] for k in ("overlay", "fixed_disparity_0", "fresh_fit")}, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
