"""Cost of linear sampling of the views' warps (stages bit 0x800) at 1920 x 1080, D = 64, default parameters.

For the synthetic frame bench.py times and the tiled real-content bud pair:
  - frame time of stages 3 against 3 | 0x800, the two alternating frame by frame in one process, HIP events around each frame
    (after a warm-up), median and mean;
  - the `synth_mux` kernel (views + interlacing, the frame's last launch) with and without the bit, alternating frame by frame
    in one profiled loop, from stm_prof_read; the nearest one is the yardstick (it is the parent commit's kernel, instruction for
    instruction);
  - how many output elements the bit changes.
usage: python tools/linwarp_time.py [--frames N] [--warmup W] [--out FILE.json] [--profile-run]
--profile-run: only a few frames of each kind (for a rocprofv3 --kernel-trace --stats or --pmc run of its own)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINEAR_WARP = 0x800


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
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    frames = {"synthetic": synth.sbs_frame(H, W, D, zd)[0], "real_content": synth.tiled_sbs_frame(bud[0], bud[1], H, W)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    both = (3, 3 | LINEAR_WARP)
    if args.profile_run:
        for sbs in frames.values():
            d_sbs = torch.from_numpy(sbs).cuda()
            for st in both * 5:
                dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
            torch.cuda.synchronize()
        print("profile run done")
        return
    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "frames": args.frames, "warmup": args.warmup}
    for name, sbs in frames.items():
        d_sbs = torch.from_numpy(sbs).cuda()
        for _ in range(args.warmup):
            for st in both:
                dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
        torch.cuda.synchronize()
        ms = {st: [] for st in both}
        for i in range(args.frames):
            for st in (both if i % 2 == 0 else both[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
                e1.record()
                e1.synchronize()
                ms[st].append(e0.elapsed_time(e1))
        r = {}
        for st, key in zip(both, ("stages3", "stages3_linwarp")):
            a = np.array(ms[st])
            r[key + "_ms_median"] = float(np.median(a))
            r[key + "_ms_mean"] = float(a.mean())
        r["frame_delta_ms_median"] = r["stages3_linwarp_ms_median"] - r["stages3_ms_median"]
        # the kernel from the library's own events, the two forms alternating frame by frame: one profiled frame at a time
        nprof = 20
        tot = {st: 0.0 for st in both}
        dev.prof_enable(True)
        for i in range(nprof):
            for st in (both if i % 2 == 0 else both[::-1]):
                dev.prof_reset()
                dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
                torch.cuda.synchronize()
                n, t = dev.prof_read("synth_mux")
                assert n == 1, n
                tot[st] += t
        dev.prof_enable(False)
        dev.prof_reset()
        r["stages3_synth_mux_ms"] = tot[3] / nprof
        r["stages3_linwarp_synth_mux_ms"] = tot[3 | LINEAR_WARP] / nprof
        r["synth_mux_ratio"] = r["stages3_linwarp_synth_mux_ms"] / r["stages3_synth_mux_ms"]
        outs = {}
        for st in both:
            dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
            torch.cuda.synchronize()
            outs[st] = out.cpu().numpy().copy()
        diff = outs[3] != outs[3 | LINEAR_WARP]
        r["output_elements_changed"] = int(np.count_nonzero(diff))
        r["output_share_changed"] = float(np.mean(diff))
        res[name] = r
        print(name, json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
