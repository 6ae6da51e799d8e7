"""Cost of the overlay compositor (stm_mux_overlay, stm_set_overlay) at 1920 x 1080, D = 64, default parameters, stages 3.

  - kernel time (stm_prof_read "overlay") of the stage call for a 120 x 1920 subtitle strip and for a full-view overlay: layout 0 in
    lens modes 0 and 2 at 1080p, and the 8 x 6 quilt at 3360 x 3360, whose full-view overlay is one 560 x 420 tile (the strip there is
    60 x 420), at disparity -8; the forms alternate, `--frames` launches each, mean;
  - the yardstick, stm_k_front (stm_prof_read "front"), from profiled frames of the same run;
  - frame time of stm_d_adcensus_stm without an overlay, with the strip and with the full-frame overlay (layout 0, lens mode 0): the
    three forms alternating frame by frame in one process, HIP events around each frame (after a warm-up), median and mean.
usage: python tools/overlay_time.py [--frames N] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PANEL = (7.37, 0.86, 0.3)
DISPARITY = -8.0
# name, N, lens, layout, (Ho, Wo), strip (rows, cols, y0), full (rows, cols)
FORMS = [("layout0_lens0_1080p", 8, None, None, (1080, 1920), (120, 1920, 900), (1080, 1920)),
         ("layout0_lens2_1080p", 8, (2,) + PANEL, None, (1080, 1920), (120, 1920, 900), (1080, 1920)),
         ("quilt_8x6_3360x3360", 48, None, (1, 8, 6, 3), (3360, 3360), (60, 420, 480), (560, 420))]


def overlay_pixels(rows, cols, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(rows, cols, 1))
    return np.concatenate([(rng.randint(0, 256, size=(rows, cols, 3)) * a + 127) // 255, a], axis=-1).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import stm_amd
    from stm_amd import device_api as dev, synth
    stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "stages": 3, "disparity": DISPARITY, "frames": args.frames, "warmup": args.warmup}

    # 1. the kernel, as a stage
    cases = []
    for name, N, lens, layout, (Ho, Wo), (sr, sc, sy), (fr, fc) in FORMS:
        frame = torch.randint(0, 256, (Ho, Wo, 3), dtype=torch.uint8, device="cuda")
        for kind, ov, y0 in (("strip", overlay_pixels(sr, sc, 1), sy), ("full", overlay_pixels(fr, fc, 2), 0)):
            cases.append((name + "_" + kind, frame, torch.from_numpy(ov).cuda(), y0, N, lens, layout, ov.shape[0] * ov.shape[1] * (Wo // fc) * (Ho // fr)))
    ms = {c[0]: 0.0 for c in cases}
    for it in range(args.warmup + args.frames):
        for key, frame, d_ov, y0, N, lens, layout, _ in cases:
            dev.prof_enable(True)
            dev.prof_reset()
            dev.d_mux_overlay(frame, d_ov, 0, y0, DISPARITY, N, 18.43, lens, layout)
            torch.cuda.synchronize()
            n, t = dev.prof_read("overlay")
            dev.prof_enable(False)
            assert n == 1
            if it >= args.warmup:
                ms[key] += t / args.frames
    res["overlay_kernel_ms"] = ms
    # bytes the compositor moves at the least: the covered frame pixels read and written (3 bytes each way) and the overlay read once per tile
    res["overlay_kernel_min_bytes"] = {c[0]: c[7] * 6 + c[2].numel() * ((c[6][1] * c[6][2]) if c[6] else 1) for c in cases}

    # 2. the frame: the yardstick kernel, and the frame time without and with the thread's overlay
    p = dev.FrameParams(num_disp=D, zero_disp=zd, num_views=8)
    d_sbs = torch.from_numpy(synth.sbs_frame(H, W, D, zd)[0]).cuda()
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    overlays = {"none": None, "strip": (cases[0][2], 900), "full": (cases[1][2], 0)}

    def frame(kind):
        if overlays[kind] is None:
            dev.set_overlay(None)
        else:
            dev.set_overlay(overlays[kind][0], 0, overlays[kind][1], DISPARITY)
        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=3)

    try:
        for _ in range(args.warmup):
            for kind in overlays:
                frame(kind)
        torch.cuda.synchronize()
        dev.prof_enable(True)
        dev.prof_reset()
        for _ in range(5):
            frame("strip")
        torch.cuda.synchronize()
        n, t = dev.prof_read("front")
        res["front_kernel_ms"] = t / n
        n, t = dev.prof_read("overlay")
        res["overlay_kernel_in_frame_ms_strip"] = t / n
        dev.prof_enable(False)
        kinds = list(overlays)
        ev = {k: [] for k in kinds}
        for i in range(args.frames):
            for kind in kinds[i % 3:] + kinds[:i % 3]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                frame(kind)
                e1.record()
                ev[kind].append((e0, e1))
        torch.cuda.synchronize()
        res["frame_ms"] = {}
        for kind in kinds:
            a = [e0.elapsed_time(e1) for e0, e1 in ev[kind]]
            res["frame_ms"][kind] = {"median": float(np.median(a)), "mean": float(np.mean(a)), "min": float(min(a)), "max": float(max(a))}
    finally:
        dev.set_overlay(None)
        dev.prof_enable(False)
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
