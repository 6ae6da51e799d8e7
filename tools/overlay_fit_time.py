"""Cost of the overlay's automatic depth placement (stm_set_overlay_auto, stm_overlay_fit) at 1920 x 1080, D = 64, default
parameters, stages 3, layout 0, lens mode 0.

Two overlays: a 120 x 1920 subtitle strip whose alpha box is about a third of its width (text in the middle, the ends transparent),
and a full-frame overlay.
  - kernel times from profiled frames (stm_prof_read): the new launches "ovfit_box" (clear + alpha box), "ovfit_hist", "ovfit_fit",
    and the compositor "overlay" with the disparity read from the state and with the setter's;
  - the yardstick, the depth budget's measurement "disp_hist" + "depth_fit" (stm_d_depth_fit on the same frame's maps), same run;
  - frame time of stm_d_adcensus_stm with the overlay at the setter's disparity and with the placement on: the forms alternating
    frame by frame in one process, HIP events around each frame (after a warm-up), median and mean.
usage: python tools/overlay_fit_time.py [--frames N] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = (-40.0, 10.0)


def overlay_pixels(rows, cols, seed, q0=0, q1=None):
    """random premultiplied pixels in columns q0 .. q1 - 1, transparent elsewhere"""
    rng = np.random.RandomState(seed)
    a = rng.randint(1, 256, size=(rows, cols, 1))
    ov = np.concatenate([(rng.randint(0, 256, size=(rows, cols, 3)) * a + 127) // 255, a], axis=-1).astype(np.uint8)
    ov[:, :q0] = 0
    if q1 is not None:
        ov[:, q1:] = 0
    return ov


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
    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "stages": 3, "limits": LIMITS, "frames": args.frames, "warmup": args.warmup,
           "placement": dict(zip(("near_permille", "margin", "pad", "rate_near", "rate_far"), dev.OVERLAY_AUTO_DEFAULTS))}
    p = dev.FrameParams(num_disp=D, zero_disp=zd, num_views=8)
    d_sbs = torch.from_numpy(synth.sbs_frame(H, W, D, zd)[0]).cuda()
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    state = torch.zeros(4, dtype=torch.float32, device="cuda")
    dstate = torch.zeros(4, dtype=torch.float32, device="cuda")
    overlays = {"strip": (torch.from_numpy(overlay_pixels(120, 1920, 1, 640, 1280)).cuda(), 900),
                "full": (torch.from_numpy(overlay_pixels(1080, 1920, 2)).cuda(), 0)}
    res["alpha_box_cols"] = {"strip": [640, 1279], "full": [0, 1919]}

    def frame(kind, auto):
        d_ov, y0 = overlays[kind]
        dev.set_overlay(d_ov, 0, y0, -8.0)
        if auto:
            dev.set_overlay_auto(LIMITS[0], LIMITS[1], state=state)
        else:
            dev.set_overlay_auto(None)
        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=3)

    forms = [(k, a) for k in overlays for a in (False, True)]
    try:
        for _ in range(args.warmup):
            for k, a in forms:
                frame(k, a)
        torch.cuda.synchronize()
        # 1. the kernels, from profiled frames
        res["kernel_ms"] = {}
        for k, a in forms:
            dev.prof_enable(True)
            dev.prof_reset()
            for _ in range(5):
                frame(k, a)
                dev.d_depth_fit(dl, dr, -8.0, 8.0, 1.0, 20, 1.0, dstate)
            torch.cuda.synchronize()
            names = ["overlay", "disp_hist", "depth_fit"] + (["ovfit_box", "ovfit_hist", "ovfit_fit"] if a else [])
            row = {}
            for name in names:
                n, t = dev.prof_read(name)
                row[name] = t / n
            dev.prof_enable(False)
            res["kernel_ms"]["%s_%s" % (k, "auto" if a else "setter")] = row
        res["state_after"] = [float(v) for v in state.cpu().numpy()]
        # 2. the frame, alternating
        ev = {f: [] for f in forms}
        for i in range(args.frames):
            for f in forms[i % 4:] + forms[:i % 4]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                frame(*f)
                e1.record()
                ev[f].append((e0, e1))
        torch.cuda.synchronize()
        res["frame_ms"] = {}
        for (k, a) in forms:
            t = [e0.elapsed_time(e1) for e0, e1 in ev[(k, a)]]
            res["frame_ms"]["%s_%s" % (k, "auto" if a else "setter")] = {"median": float(np.median(t)), "mean": float(np.mean(t)),
                                                                          "min": float(min(t)), "max": float(max(t))}
        res["frame_delta_ms_median"] = {k: res["frame_ms"][k + "_auto"]["median"] - res["frame_ms"][k + "_setter"]["median"] for k in overlays}
    finally:
        dev.set_overlay_auto(None)
        dev.set_overlay(None)
        dev.prof_enable(False)
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
