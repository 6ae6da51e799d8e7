"""Cost of the lenticular interlacer (stm_set_lens) at 1920 x 1080, D = 64, default parameters, panel pitch 7.37 / slope 0.86 /
centre 0.3.

For the synthetic frame bench.py times and the tiled real-content bud pair:
  - frame time of stages 3 | 0x800 under modes 0 (the reference's interlacer), 1, 2 and 3, the four alternating frame by frame in one
    process, HIP events around each frame (after a warm-up), median and mean;
  - the `synth_mux` kernel (views + interlacing, the frame's last launch) of each mode, alternating frame by frame in one profiled
    loop, from stm_prof_read; mode 0 is the yardstick (it is the parent commit's kernel, instruction for instruction);
  - how many output elements each mode changes against mode 0, and mode 3 against mode 1.
usage: python tools/lens_time.py [--frames N] [--warmup W] [--out FILE.json] [--profile-run]
--profile-run: only a few frames of each mode (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINEAR_WARP = 0x800
PANEL = (7.37, 0.86, 0.3)
MODES = (0, 1, 2, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    args = ap.parse_args()
    import torch
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, synth
    stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    stages = 3 | LINEAR_WARP
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    frames = {"synthetic": synth.sbs_frame(H, W, D, zd)[0], "real_content": synth.tiled_sbs_frame(bud[0], bud[1], H, W)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")

    def frame(d_sbs, mode):
        dev.set_lens(mode, *PANEL)
        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=stages)

    try:
        if args.profile_run:
            for sbs in frames.values():
                d_sbs = torch.from_numpy(sbs).cuda()
                for mode in MODES * 5:
                    frame(d_sbs, mode)
                torch.cuda.synchronize()
            print("profile run done")
            return
        res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "stages": stages, "panel": list(PANEL), "frames": args.frames,
               "warmup": args.warmup}
        for name, sbs in frames.items():
            d_sbs = torch.from_numpy(sbs).cuda()
            for _ in range(args.warmup):
                for mode in MODES:
                    frame(d_sbs, mode)
            torch.cuda.synchronize()
            ms = {mode: [] for mode in MODES}
            for i in range(args.frames):
                for mode in MODES[i % 4:] + MODES[:i % 4]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    frame(d_sbs, mode)
                    e1.record()
                    e1.synchronize()
                    ms[mode].append(e0.elapsed_time(e1))
            r = {}
            for mode in MODES:
                a = np.array(ms[mode])
                r["mode%d_frame_ms_median" % mode] = float(np.median(a))
                r["mode%d_frame_ms_mean" % mode] = float(a.mean())
            # the kernel from the library's own events, the modes alternating frame by frame: one profiled frame at a time
            nprof = 20
            tot = {mode: 0.0 for mode in MODES}
            dev.prof_enable(True)
            for i in range(nprof):
                for mode in MODES[i % 4:] + MODES[:i % 4]:
                    dev.prof_reset()
                    frame(d_sbs, mode)
                    torch.cuda.synchronize()
                    n, t = dev.prof_read("synth_mux")
                    assert n == 1, n
                    tot[mode] += t
            dev.prof_enable(False)
            dev.prof_reset()
            outs = {}
            for mode in MODES:
                frame(d_sbs, mode)
                torch.cuda.synchronize()
                outs[mode] = out.cpu().numpy().copy()
            for mode in MODES:
                r["mode%d_synth_mux_ms" % mode] = tot[mode] / nprof
                if mode:
                    r["mode%d_synth_mux_ratio" % mode] = tot[mode] / tot[0]
                    r["mode%d_frame_delta_ms_median" % mode] = r["mode%d_frame_ms_median" % mode] - r["mode0_frame_ms_median"]
                    r["mode%d_output_share_changed" % mode] = float(np.mean(outs[mode] != outs[0]))
            r["mode3_vs_mode1_output_share_changed"] = float(np.mean(outs[3] != outs[1]))
            res[name] = r
            print(name, json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        dev.set_lens(0)


if __name__ == "__main__":
    main()
