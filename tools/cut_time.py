"""Cost of the shot-change detector (stm_set_cut) at 1920 x 1080, D = 64, default parameters, stages 3.

For the synthetic frame bench.py times, the tiled real-content bud pair, a flat frame (every lane of the signature kernel hits one
bin) and a noise frame, as BGR; and for the synthetic frame as NV12 and as a half-width side-by-side frame (linear filter):
  - the two scopes `cut_sig` (the clear and the signature kernel) and `cut_decide` inside profiled frames of stm_d_adcensus_stm /
    _nv12 with the detector on and the colour balance in mode 2, beside `balance_hist` (stm_k_balance_hist with its clear: it reads
    both eyes and counts six values per pixel where the signature reads one eye and counts one) and `front` (stm_k_front) from the
    same frames, from stm_prof_read;
  - the frame time with the detector off and on (nothing else set), the two alternating frame by frame in one process, HIP events
    around each frame (after a warm-up), median and mean.
usage: python tools/cut_time.py [--frames N] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("cut_sig", "cut_decide", "balance_hist", "front")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, synth, video
    stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    syn = synth.sbs_frame(H, W, D, zd)[0]
    inputs = [("bgr_synthetic", "bgr", syn, None),
              ("bgr_real_content", "bgr", synth.tiled_sbs_frame(bud[0], bud[1], H, W), None),
              ("bgr_flat", "bgr", np.full((H, 2 * W, 3), 128, np.uint8), None),
              ("bgr_noise", "bgr", np.random.RandomState(1).randint(0, 256, size=(H, 2 * W, 3)).astype(np.uint8), None),
              ("nv12_synthetic", "nv12", synth.bgr_to_nv12(syn, 0), None),
              ("half_width_synthetic", "bgr", synth.pack_frame(syn[:, :W], syn[:, W:], 1, 0, 0), (1, 0, 0, 0))]
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    cut_state = torch.zeros(260, dtype=torch.int32, device="cuda")
    bal_state = torch.zeros(769, dtype=torch.int32, device="cuda")
    thresh = video.CUT_DEFAULT[0]

    def frame(kind, d_in, on):
        if on:
            dev.set_cut(1, thresh, 1, cut_state)
        else:
            dev.set_cut(0)
        if kind == "nv12":
            dev.d_adcensus_stm_nv12(d_in[0], d_in[1], dl, dr, out, p, 3, 0)
        else:
            dev.d_adcensus_stm(d_in, dl, dr, out, p, stages=3)

    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "stages": 3, "thresh_permille": thresh, "frames": args.frames, "warmup": args.warmup}
    try:
        for name, kind, inp, pk in inputs:
            d_in = tuple(torch.from_numpy(a).cuda() for a in inp) if kind == "nv12" else torch.from_numpy(inp).cuda()
            if pk is not None:
                dev.set_packing(*pk)
            r = {}
            nprof = 20
            dev.set_balance_auto(48, 1.0, bal_state)
            dev.set_balance(2)
            dev.prof_enable(True)
            frame(kind, d_in, True)  # (not timed)
            tot = {k: 0.0 for k in KERNELS}
            for _ in range(nprof):
                dev.prof_reset()
                frame(kind, d_in, True)
                torch.cuda.synchronize()
                for k in KERNELS:
                    n, t = dev.prof_read(k)
                    assert n == 1, (k, n)
                    tot[k] += t
            for k in KERNELS:
                r[k + "_ms"] = tot[k] / nprof
            r["cut_sig_vs_balance_hist"] = tot["cut_sig"] / tot["balance_hist"]
            dev.prof_enable(False)
            dev.prof_reset()
            dev.set_balance(0)
            dev.set_balance_auto(48, 1.0, None)
            r["state_head"] = [int(v) for v in cut_state.cpu().numpy()[:4]]
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
            dev.set_packing(0, 0, 0, 0)
            res[name] = r
            print(name, json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        dev.set_cut(0)
        dev.set_packing(0, 0, 0, 0)
        dev.set_balance(0)
        dev.set_balance_auto(48, 1.0, None)


if __name__ == "__main__":
    main()
