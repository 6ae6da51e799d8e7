"""Cost of the active picture area (stm_set_active mode 2) at 1920 x 1080, D = 64, default parameters, stages 3.

For the synthetic frame bench.py times inside a 2.39:1 letterbox (136 rows of levels 0 .. 3 top and bottom), the same frame without
bars, and a noise frame (every pixel lit: the most adds the count kernel can make), as BGR; and for the letterboxed frame as NV12:
  - the three scopes `active_clear`, `active_count` and `active_decide` inside profiled frames of stm_d_adcensus_stm / _nv12 with the
    active area in mode 2 and the shot-change detector on, beside `cut_sig` (stm_k_cut_sig with its clear: the same input, read the
    same way, with a histogram add per pixel where the count kernel has a ballot) and `cut_decide` from the same frames, from
    stm_prof_read;
  - the frame time with the active area off and on (nothing else set), the two alternating frame by frame in one process, HIP events
    around each frame (after a warm-up), median and mean.
usage: python tools/active_time.py [--frames N] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("active_clear", "active_count", "active_decide", "cut_sig", "cut_decide")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import stm_amd
    from stm_amd import device_api as dev, synth, video
    stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    syn = synth.sbs_frame(H, W, D, zd)[0]
    boxed = syn.copy()
    rng = np.random.RandomState(1)
    boxed[:136] = rng.randint(0, 4, size=boxed[:136].shape)
    boxed[H - 136:] = rng.randint(0, 4, size=boxed[H - 136:].shape)
    inputs = [("bgr_letterbox", "bgr", boxed), ("bgr_no_bars", "bgr", syn),
              ("bgr_noise", "bgr", np.random.RandomState(2).randint(0, 256, size=(H, 2 * W, 3)).astype(np.uint8)),
              ("nv12_letterbox", "nv12", synth.bgr_to_nv12(boxed, 0))]
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    cut_state = torch.zeros(260, dtype=torch.int32, device="cuda")
    act_state = torch.zeros(16, dtype=torch.int32, device="cuda")

    def frame(kind, d_in, on, cut=False):
        dev.set_active(2 if on else 0)
        if cut:
            dev.set_cut(1, video.CUT_DEFAULT[0], 1, cut_state)
        else:
            dev.set_cut(0)
        if kind == "nv12":
            dev.d_adcensus_stm_nv12(d_in[0], d_in[1], dl, dr, out, p, 3, 0)
        else:
            dev.d_adcensus_stm(d_in, dl, dr, out, p, stages=3)

    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "stages": 3, "detector": list(video.ACTIVE_AUTO_DEFAULT), "frames": args.frames,
           "warmup": args.warmup}
    try:
        dev.set_active_auto(*video.ACTIVE_AUTO_DEFAULT, act_state)
        for name, kind, inp in inputs:
            d_in = tuple(torch.from_numpy(a).cuda() for a in inp) if kind == "nv12" else torch.from_numpy(inp).cuda()
            r = {}
            nprof = 20
            act_state.zero_()
            dev.prof_enable(True)
            frame(kind, d_in, True, True)  # (not timed)
            tot = {k: 0.0 for k in KERNELS}
            for _ in range(nprof):
                dev.prof_reset()
                frame(kind, d_in, True, True)
                torch.cuda.synchronize()
                for k in KERNELS:
                    n, t = dev.prof_read(k)
                    assert n == 1, (k, n)
                    tot[k] += t
            for k in KERNELS:
                r[k + "_ms"] = tot[k] / nprof
            r["active_count_vs_cut_sig"] = tot["active_count"] / tot["cut_sig"]
            dev.prof_enable(False)
            dev.prof_reset()
            r["state"] = [int(v) for v in act_state.cpu().numpy()]
            for _ in range(args.warmup):
                frame(kind, d_in, False)
                frame(kind, d_in, True)
            torch.cuda.synchronize()
            ms = {False: [], True: []}
            for i in range(args.frames):
                for on in ((False, True), (True, False))[i % 2]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    frame(kind, d_in, on)
                    e1.record()
                    e1.synchronize()
                    ms[on].append(e0.elapsed_time(e1))
            for on, label in ((False, "off"), (True, "on")):
                a = np.array(ms[on])
                r["frame_ms_median_" + label] = float(np.median(a))
                r["frame_ms_mean_" + label] = float(a.mean())
            r["frame_delta_ms_median"] = r["frame_ms_median_on"] - r["frame_ms_median_off"]
            res[name] = r
            print(name, json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        dev.set_active(0)
        dev.set_active_auto()
        dev.set_cut(0)


if __name__ == "__main__":
    main()
