"""Cost of the outlier interpolation (stages bit 0x400) at 1920 x 1080, D = 64, default parameters.

For the synthetic frame bench.py times and the tiled real-content bud pair:
  - frame time of stages 3 against 3 | 0x400, the two alternating frame by frame in one process, HIP events around each frame
    (after a warm-up), median and mean;
  - the `interp` kernel (both views, one launch) next to the yardstick, the region-voting kernels `irv` of the same frame, and
    the `bilateral` kernel, from stm_prof_read (a separate, profiled loop);
  - how many pixels the step visits: the outliers after the L/R check and after region voting x5, per view (the oracle's DCC +
    IRV on the GPU's WTA maps), and how many of them the step changes.
usage: python tools/interp_time.py [--frames N] [--warmup W] [--out FILE.json] [--profile-run]
--profile-run: only a few frames of each kind (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INTERP = 0x400


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
    if args.profile_run:
        for sbs in frames.values():
            d_sbs = torch.from_numpy(sbs).cuda()
            for st in (3, 3 | INTERP) * 5:
                dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
            torch.cuda.synchronize()
        print("profile run done")
        return
    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "frames": args.frames, "warmup": args.warmup}
    for name, sbs in frames.items():
        d_sbs = torch.from_numpy(sbs).cuda()
        for _ in range(args.warmup):
            for st in (3, 3 | INTERP):
                dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
        torch.cuda.synchronize()
        ms = {3: [], 3 | INTERP: []}
        for i in range(args.frames):
            for st in ((3, 3 | INTERP) if i % 2 == 0 else (3 | INTERP, 3)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
                e1.record()
                e1.synchronize()
                ms[st].append(e0.elapsed_time(e1))
        r = {}
        for st, key in ((3, "stages3"), (3 | INTERP, "stages3_interp")):
            a = np.array(ms[st])
            r[key + "_ms_median"] = float(np.median(a))
            r[key + "_ms_mean"] = float(a.mean())
        r["frame_delta_ms_median"] = r["stages3_interp_ms_median"] - r["stages3_ms_median"]
        # kernel times from the library's own events: per frame, all launches of a name summed (irv: the whole voting chain)
        nprof = 20
        for st, key in ((3, "stages3"), (3 | INTERP, "stages3_interp")):
            dev.prof_reset()
            dev.prof_enable(True)
            for _ in range(nprof):
                dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
            torch.cuda.synchronize()
            dev.prof_enable(False)
            for k in ("interp", "irv", "bilateral"):
                n, t = dev.prof_read(k)
                if n:
                    r["%s_%s_ms_per_frame" % (key, k)] = t / nprof
        dev.prof_reset()
        # the pixels the step visits (the oracle's DCC + IRV on the GPU's WTA maps are bit-identical to the frame's own)
        from oracle import pyoracle as orc
        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=1)
        torch.cuda.synchronize()
        wl, wr = dl.cpu().numpy(), dr.cpu().numpy()
        L, R = orc.demux_sbs(sbs, W)
        ol, orr = orc.dr_dcc(wl, wr)
        r["outliers_after_dcc"] = [int(np.count_nonzero(ol)), int(np.count_nonzero(orr))]
        changed, after = [], []
        for img, w, o in ((L, wl, ol), (R, wr, orr)):
            x = orc.cross_arms(img, p.ucd, p.lcd, p.usd, p.lsd)
            w, o = orc.dr_irv(w, o, x, p.thresh_s, p.thresh_h, D, zd, p.usd, 5, device_flavour=True)
            after.append(int(np.count_nonzero(o)))
            d_w = torch.from_numpy(w).cuda()
            dev.d_dr_interp(d_w, torch.from_numpy(o).cuda(), torch.from_numpy(img).cuda())
            torch.cuda.synchronize()
            changed.append(int(np.count_nonzero(d_w.cpu().numpy() != w)))
        r["outliers_after_irv"] = after
        r["outlier_share_of_image"] = float(sum(after)) / (2.0 * H * W)
        r["pixels_changed"] = changed
        res[name] = r
        print(name, json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
