"""Cost of the vertical alignment (stm_set_align) at 1920 x 1080, D = 64, default parameters, stages 3, radius 16.

For the synthetic frame bench.py times and the tiled real-content bud pair, the right eye of each displaced by (3.3, 0.002, -0.004):
  - the four kernels `align_profiles`, `align_sad`, `align_fit` and `align_frame` inside profiled frames of stm_d_adcensus_stm in
    mode 2, and `front` (stm_k_front, the yardstick: the same traffic class as align_frame, both images read and written once) from
    the same frames, from stm_prof_read;
  - the field the measurement found;
  - the frame time with the setting off, in mode 1 (the apply pass alone) and in mode 2, the three alternating frame by frame in one
    process, HIP events around each frame (after a warm-up), median and mean.
usage: python tools/align_time.py [--frames N] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELD = (3.3, 0.002, -0.004)
RADIUS = 16
KERNELS = ("align_profiles", "align_sad", "align_fit", "align_frame", "front")


def displace_right(sbs, a, b, c):
    """the right half of a side-by-side frame resampled so that its content lies dy = a + b u + c v rows lower (float bilinear)"""
    H, W2 = sbs.shape[:2]
    W = W2 // 2
    img = sbs[:, W:].astype(np.float64)
    u = np.arange(W, dtype=np.float64)[None, :] - (W - 1) / 2.0
    v = np.arange(H, dtype=np.float64)[:, None] - (H - 1) / 2.0
    s = np.arange(H, dtype=np.float64)[:, None] - (a + b * u + c * v)
    s0 = np.floor(s)
    fr = (s - s0)[:, :, None]
    r0 = np.clip(s0.astype(np.int64), 0, H - 1)
    r1 = np.clip(s0.astype(np.int64) + 1, 0, H - 1)
    cols = np.broadcast_to(np.arange(W)[None, :], (H, W))
    out = sbs.copy()
    out[:, W:] = np.clip(np.floor((1.0 - fr) * img[r0, cols] + fr * img[r1, cols] + 0.5), 0, 255).astype(np.uint8)
    return out


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
    frames = {"synthetic": displace_right(synth.sbs_frame(H, W, D, zd)[0], *FIELD),
              "real_content": displace_right(synth.tiled_sbs_frame(bud[0], bud[1], H, W), *FIELD)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    state = torch.zeros(4, dtype=torch.float32, device="cuda")
    dev.set_align_auto(RADIUS, 1.0, state)

    def frame(d_sbs, mode):
        dev.set_align(mode, *FIELD)
        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=3)

    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "stages": 3, "field": list(FIELD), "radius": RADIUS, "frames": args.frames,
           "warmup": args.warmup}
    try:
        for name, sbs in frames.items():
            d_sbs = torch.from_numpy(sbs).cuda()
            r = {}
            nprof = 20
            dev.prof_enable(True)
            frame(d_sbs, 2)  # (not timed)
            tot = {k: 0.0 for k in KERNELS}
            for _ in range(nprof):
                dev.prof_reset()
                frame(d_sbs, 2)
                torch.cuda.synchronize()
                for k in KERNELS:
                    n, t = dev.prof_read(k)
                    assert n == 1, (k, n)
                    tot[k] += t
            for k in KERNELS:
                r[k + "_ms"] = tot[k] / nprof
            r["align_total_vs_front"] = sum(tot[k] for k in KERNELS[:4]) / tot["front"]
            dev.prof_enable(False)
            dev.prof_reset()
            r["state"] = [float(v) for v in state.cpu().numpy()]
            for _ in range(args.warmup):
                for m in (0, 1, 2):
                    frame(d_sbs, m)
            torch.cuda.synchronize()
            ms = {0: [], 1: [], 2: []}
            for i in range(args.frames):
                for m in ((0, 1, 2), (1, 2, 0), (2, 0, 1))[i % 3]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    frame(d_sbs, m)
                    e1.record()
                    e1.synchronize()
                    ms[m].append(e0.elapsed_time(e1))
            for m, label in ((0, "off"), (1, "manual"), (2, "auto")):
                a = np.array(ms[m])
                r["frame_ms_median_" + label] = float(np.median(a))
                r["frame_ms_mean_" + label] = float(a.mean())
            r["frame_delta_ms_median_manual"] = r["frame_ms_median_manual"] - r["frame_ms_median_off"]
            r["frame_delta_ms_median_auto"] = r["frame_ms_median_auto"] - r["frame_ms_median_off"]
            res[name] = r
            print(name, json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        dev.set_align(0)
        dev.set_align_auto(16, 1.0, None)


if __name__ == "__main__":
    main()
