"""Cost of view antialiasing (stm_set_antialias) at 1920 x 1080, D = 64, default parameters, stages 3.

For the synthetic frame bench.py times and the tiled real-content bud pair:
  - the `prefilter` kernel (both images in one launch) with everything passed through (strength 0) and at strength 1, max_radius 8,
    gate 1, and `front` (stm_k_front, the yardstick: the same traffic class, both images read and written once) in the same profiled
    run, from stm_prof_read;
  - the share of pixels the second setting blurs (H != 0), from the frame's own maps;
  - the frame time with the setting off and on, the two alternating frame by frame in one process, HIP events around each frame
    (after a warm-up), median and mean.
usage: python tools/antialias_time.py [--frames N] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = {"pass_through": (0.0, 8, 1.0), "strength_1": (1.0, 8, 1.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, synth
    stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    frames = {"synthetic": synth.sbs_frame(H, W, D, zd)[0], "real_content": synth.tiled_sbs_frame(bud[0], bud[1], H, W)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")

    def frame(d_sbs, setting):
        if setting is None:
            dev.set_antialias(0)
        else:
            dev.set_antialias(1, *setting)
        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=3)

    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "stages": 3, "settings": {k: list(v) for k, v in SETTINGS.items()},
           "frames": args.frames, "warmup": args.warmup}
    try:
        for name, sbs in frames.items():
            d_sbs = torch.from_numpy(sbs).cuda()
            r = {}
            nprof = 20
            dev.prof_enable(True)
            for label, setting in SETTINGS.items():
                frame(d_sbs, setting)  # (not timed)
                pre = front = 0.0
                for _ in range(nprof):
                    dev.prof_reset()
                    frame(d_sbs, setting)
                    torch.cuda.synchronize()
                    n, t = dev.prof_read("prefilter")
                    assert n == 1, n
                    pre += t
                    n, t = dev.prof_read("front")
                    assert n == 1, n
                    front += t
                r[label + "_prefilter_ms"] = pre / nprof
                r[label + "_front_ms"] = front / nprof
                r[label + "_prefilter_vs_front"] = pre / front
            dev.prof_enable(False)
            dev.prof_reset()
            k16 = np.float32(SETTINGS["strength_1"][0] * 8.0 / (p.num_views - 1))
            h = np.abs(torch.stack([dl, dr]).cpu().numpy()) * k16 + np.float32(0.5)
            r["strength_1_blurred_share"] = float((h >= 1.0).mean())
            order = [None, SETTINGS["strength_1"]]
            for _ in range(args.warmup):
                for s in order:
                    frame(d_sbs, s)
            torch.cuda.synchronize()
            ms = {0: [], 1: []}
            for i in range(args.frames):
                for k in ((0, 1) if i % 2 == 0 else (1, 0)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    frame(d_sbs, order[k])
                    e1.record()
                    e1.synchronize()
                    ms[k].append(e0.elapsed_time(e1))
            for k, label in ((0, "off"), (1, "on")):
                a = np.array(ms[k])
                r["frame_ms_median_" + label] = float(np.median(a))
                r["frame_ms_mean_" + label] = float(a.mean())
            r["frame_delta_ms_median"] = r["frame_ms_median_on"] - r["frame_ms_median_off"]
            res[name] = r
            print(name, json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        dev.set_antialias(0)


if __name__ == "__main__":
    main()
