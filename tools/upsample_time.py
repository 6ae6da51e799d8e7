"""Cost of the guided disparity up-sampling (stages bit 0x1000 of the reduced-resolution frame) at 1920 x 1080 matched at
960 x 540, D = 64, default parameters.

For the synthetic frame bench.py times and the tiled real-content bud pair:
  - frame time of stm_d_adcensus_stm_2s with stages 3 against 3 | 0x1000, the two alternating frame by frame in one process, HIP
    events around each frame (after a warm-up), median and mean;
  - the `upsample` kernel (one launch, both views) against the two `disp_scale` launches it replaces, alternating frame by frame
    in one profiled loop, from stm_prof_read; the bilinear pair is the yardstick (it is the parent commit's kernel);
  - how many map elements the bit changes, and by how much.
usage: python tools/upsample_time.py [--frames N] [--warmup W] [--out FILE.json] [--profile-run]
--profile-run: only a few frames of each kind (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GUIDED_UP = 0x1000


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
    H, W, h, w, D, zd = 1080, 1920, 540, 960, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    frames = {"synthetic": synth.sbs_frame(H, W, D, zd)[0], "real_content": synth.tiled_sbs_frame(bud[0], bud[1], H, W)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    both = (3, 3 | GUIDED_UP)

    def frame(d_sbs, st):
        dev.d_adcensus_stm_2s(d_sbs, dl, dr, out, p, h, w, 0.5, stages=st)

    if args.profile_run:
        for sbs in frames.values():
            d_sbs = torch.from_numpy(sbs).cuda()
            for st in both * 5:
                frame(d_sbs, st)
            torch.cuda.synchronize()
        print("profile run done")
        return
    res = {"shape": [H, W], "match_shape": [h, w], "num_disp": D, "zero_disp": zd, "frames": args.frames, "warmup": args.warmup}
    for name, sbs in frames.items():
        d_sbs = torch.from_numpy(sbs).cuda()
        for _ in range(args.warmup):
            for st in both:
                frame(d_sbs, st)
        torch.cuda.synchronize()
        ms = {st: [] for st in both}
        for i in range(args.frames):
            for st in (both if i % 2 == 0 else both[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                frame(d_sbs, st)
                e1.record()
                e1.synchronize()
                ms[st].append(e0.elapsed_time(e1))
        r = {}
        for st, key in zip(both, ("stages3", "stages3_guided")):
            a = np.array(ms[st])
            r[key + "_ms_median"] = float(np.median(a))
            r[key + "_ms_mean"] = float(a.mean())
        r["frame_delta_ms_median"] = r["stages3_guided_ms_median"] - r["stages3_ms_median"]
        r["frame_delta_share"] = r["frame_delta_ms_median"] / r["stages3_ms_median"]
        # the kernels from the library's own events, the two forms alternating frame by frame: one profiled frame at a time
        nprof = 20
        t_scale, t_up = 0.0, 0.0
        dev.prof_enable(True)
        for i in range(nprof):
            for st in (both if i % 2 == 0 else both[::-1]):
                dev.prof_reset()
                frame(d_sbs, st)
                torch.cuda.synchronize()
                n_s, ts = dev.prof_read("disp_scale")
                n_u, tu = dev.prof_read("upsample")
                assert (n_s, n_u) == ((2, 0) if st == 3 else (0, 1)), (st, n_s, n_u)
                t_scale += ts
                t_up += tu
        dev.prof_enable(False)
        dev.prof_reset()
        r["disp_scale_pair_ms"] = t_scale / nprof
        r["upsample_ms"] = t_up / nprof
        r["kernel_ratio"] = r["upsample_ms"] / r["disp_scale_pair_ms"]
        maps = {}
        for st in both:
            frame(d_sbs, st)
            torch.cuda.synchronize()
            maps[st] = dl.cpu().numpy().copy()
        diff = np.abs(maps[3] - maps[3 | GUIDED_UP])
        r["left_map_elements_changed"] = int(np.count_nonzero(diff))
        r["left_map_share_changed"] = float(np.mean(diff != 0))
        r["left_map_share_changed_by_more_than_1"] = float(np.mean(diff > 1))
        res[name] = r
        print(name, json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
