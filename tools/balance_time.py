"""Cost of the colour balance between the eyes (stm_set_balance) at 1920 x 1080, D = 64, default parameters, stages 3, max_shift 48.

For the synthetic frame bench.py times, the tiled real-content bud pair (the right eye of both distorted by gain (0.8, 0.95, 0.9),
offset (10, -5, 4), gamma (0.85, 1.1, 1.2)), a flat frame (every lane of the histogram kernel hits one bin per channel) and a noise
frame (every lane another bin):
  - the three kernels `balance_hist` (with its clear launch), `balance_fit` and `balance_frame` inside profiled frames of
    stm_d_adcensus_stm in mode 2 with a manual alignment on as well, beside `align_frame` and `front` (stm_k_front, the yardstick:
    the same traffic class as the apply passes, both images read and written once) from the same frames, from stm_prof_read;
  - the histogram kernel's flat-against-noise ratio: the evidence for how the LDS counting handles contention;
  - the frame time with the setting off, in mode 1 (the apply pass alone) and in mode 2, the three alternating frame by frame in one
    process, HIP events around each frame (after a warm-up), median and mean.
usage: python tools/balance_time.py [--frames N] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTING = ((0.8, 0.95, 0.9), (10, -5, 4), (0.85, 1.1, 1.2))
FIELD = (3.3, 0.002, -0.004)
MAX_SHIFT = 48
KERNELS = ("balance_hist", "balance_fit", "balance_frame", "align_frame", "front")


def distort_right(sbs, gain, offset, gamma):
    """the right half of a side-by-side frame through floor(255 (x/255)^gamma * gain + offset + 0.5) per channel, clipped"""
    W = sbs.shape[1] // 2
    out = sbs.copy()
    x = np.arange(256, dtype=np.float64)
    for c in range(3):
        curve = np.clip(np.floor(255.0 * (x / 255.0) ** gamma[c] * gain[c] + offset[c] + 0.5), 0, 255).astype(np.uint8)
        out[:, W:, c] = curve[sbs[:, W:, c]]
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
    frames = {"synthetic": distort_right(synth.sbs_frame(H, W, D, zd)[0], *SETTING),
              "real_content": distort_right(synth.tiled_sbs_frame(bud[0], bud[1], H, W), *SETTING),
              "flat": np.full((H, 2 * W, 3), 128, np.uint8),
              "noise": np.random.RandomState(1).randint(0, 256, size=(H, 2 * W, 3)).astype(np.uint8)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    state = torch.zeros(769, dtype=torch.int32, device="cuda")
    given = np.tile(np.clip(np.arange(256) * 1.1 - 4, 0, 255).astype(np.uint8), (3, 1))
    dev.set_balance_auto(MAX_SHIFT, 1.0, state)

    def frame(d_sbs, mode):
        dev.set_balance(mode, given if mode == 1 else None)
        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=3)

    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "stages": 3, "setting": [list(v) for v in SETTING], "max_shift": MAX_SHIFT,
           "align_field_in_profiled_frames": list(FIELD), "frames": args.frames, "warmup": args.warmup}
    try:
        for name, sbs in frames.items():
            d_sbs = torch.from_numpy(sbs).cuda()
            r = {}
            nprof = 20
            dev.set_align(1, *FIELD)
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
            r["balance_total_vs_front"] = sum(tot[k] for k in KERNELS[:3]) / tot["front"]
            dev.prof_enable(False)
            dev.prof_reset()
            dev.set_align(0)
            st = state.cpu().numpy()
            r["tables_at_64_128_192"] = [[int(np.clip((int(st[1 + c * 256 + v]) + 128) >> 8, 0, 255)) for v in (64, 128, 192)] for c in range(3)]
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
            for m, label in ((0, "off"), (1, "given"), (2, "measured")):
                a = np.array(ms[m])
                r["frame_ms_median_" + label] = float(np.median(a))
                r["frame_ms_mean_" + label] = float(a.mean())
            r["frame_delta_ms_median_given"] = r["frame_ms_median_given"] - r["frame_ms_median_off"]
            r["frame_delta_ms_median_measured"] = r["frame_ms_median_measured"] - r["frame_ms_median_off"]
            res[name] = r
            print(name, json.dumps(r), flush=True)
        res["balance_hist_flat_vs_noise"] = res["flat"]["balance_hist_ms"] / res["noise"]["balance_hist_ms"]
        print("balance_hist flat / noise:", res["balance_hist_flat_vs_noise"], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        dev.set_align(0)
        dev.set_balance(0)
        dev.set_balance_auto(48, 1.0, None)


if __name__ == "__main__":
    main()
