"""Cost of the depth budget (stm_set_depth) at 1920 x 1080, D = 64, default parameters, stages 3 | 0x800, under the reference's
interlacer (lens mode 0) and the panel pitch 7.37 / slope 0.86 / centre 0.3 in lens mode 3.

For the synthetic frame bench.py times and the tiled real-content bud pair:
  - frame time with the depth budget off, manual (gain 0.5, conv 2) and automatic (budget [-8, 8], clip 20, rate 0.25, a caller-owned
    state), the configurations alternating frame by frame in one process, HIP events around each frame (after a warm-up), median
    and mean;
  - the `synth_mux` kernel of each configuration and the `disp_hist` (clear + histogram) and `depth_fit` kernels of the automatic
    one, alternating frame by frame in one profiled loop, from stm_prof_read; depth off is the yardstick (the parent commit's kernel);
  - the gain and convergence the automatic mode settles on;
  - the rate of a frame stream (zero-copy submit / collect, frames per second) with depth off and with the automatic mode, whose
    frames run one after the other on the GPU.
usage: python tools/depth_time.py [--frames N] [--warmup W] [--stream-frames M] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINEAR_WARP = 0x800
PANEL = (7.37, 0.86, 0.3)
MANUAL = (0.5, 2.0)
AUTO = (-8.0, 8.0, 1.0, 20, 0.25)
CONFIGS = [(lens, depth) for lens in (0, 3) for depth in (0, 1, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--stream-frames", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, synth, video
    stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    stages = 3 | LINEAR_WARP
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    frames = {"synthetic": synth.sbs_frame(H, W, D, zd)[0], "real_content": synth.tiled_sbs_frame(bud[0], bud[1], H, W)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    state = torch.zeros(4, dtype=torch.float32, device="cuda")
    dev.set_depth_auto(*AUTO, state)

    def frame(d_sbs, cfg):
        lens, depth = cfg
        dev.set_lens(lens, *PANEL)
        dev.set_depth(depth, *MANUAL)
        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=stages)

    def rot(i):
        k = i % len(CONFIGS)
        return CONFIGS[k:] + CONFIGS[:k]

    def key(cfg):
        return "lens%d_depth%d" % cfg

    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "stages": stages, "panel": list(PANEL), "manual": list(MANUAL),
           "auto": list(AUTO), "frames": args.frames, "warmup": args.warmup}
    try:
        for name, sbs in frames.items():
            d_sbs = torch.from_numpy(sbs).cuda()
            state.zero_()
            for _ in range(args.warmup):
                for cfg in CONFIGS:
                    frame(d_sbs, cfg)
            torch.cuda.synchronize()
            ms = {cfg: [] for cfg in CONFIGS}
            for i in range(args.frames):
                for cfg in rot(i):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    frame(d_sbs, cfg)
                    e1.record()
                    e1.synchronize()
                    ms[cfg].append(e0.elapsed_time(e1))
            r = {}
            for cfg in CONFIGS:
                a = np.array(ms[cfg])
                r[key(cfg) + "_frame_ms_median"] = float(np.median(a))
                r[key(cfg) + "_frame_ms_mean"] = float(a.mean())
            nprof = 20
            tot = {cfg: 0.0 for cfg in CONFIGS}
            hist_ms = fit_ms = 0.0
            dev.prof_enable(True)
            for i in range(nprof):
                for cfg in rot(i):
                    dev.prof_reset()
                    frame(d_sbs, cfg)
                    torch.cuda.synchronize()
                    n, t = dev.prof_read("synth_mux")
                    assert n == 1, n
                    tot[cfg] += t
                    if cfg[1] == 2:
                        n, t = dev.prof_read("disp_hist")
                        assert n == 1, n
                        hist_ms += t
                        n, t = dev.prof_read("depth_fit")
                        assert n == 1, n
                        fit_ms += t
            dev.prof_enable(False)
            dev.prof_reset()
            for cfg in CONFIGS:
                r[key(cfg) + "_synth_mux_ms"] = tot[cfg] / nprof
                if cfg[1]:
                    base = (cfg[0], 0)
                    r[key(cfg) + "_synth_mux_ratio"] = tot[cfg] / tot[base]
                    r[key(cfg) + "_frame_delta_ms_median"] = r[key(cfg) + "_frame_ms_median"] - r[key(base) + "_frame_ms_median"]
            r["lens3_vs_lens0_synth_mux_ratio_depth_off"] = tot[(3, 0)] / tot[(0, 0)]
            r["disp_hist_ms"] = hist_ms / (2 * nprof)
            r["depth_fit_ms"] = fit_ms / (2 * nprof)
            st = state.cpu().numpy()
            r["auto_gain"], r["auto_conv"] = float(st[1]), float(st[2])
            dev.set_lens(0)
            dev.set_depth(0)
            # the frame stream, zero-copy: frames per second with the depth budget off and automatic
            for label, kw in (("off", {}), ("auto", {"depth_auto": AUTO})):
                fs = video.FrameStream(H, W, p, stages=stages, **kw)
                n_done, pending, t0 = 0, 0, None
                for k in range(args.stream_frames + 8):
                    if k == 8:
                        t0 = time.perf_counter()
                    if pending == 2:
                        fs.collect_view()
                        pending -= 1
                        n_done += 1
                    fs.input_buffer()[...] = sbs
                    fs.submit_inplace()
                    pending += 1
                while pending:
                    fs.collect_view()
                    pending -= 1
                r["stream_fps_depth_" + label] = args.stream_frames / (time.perf_counter() - t0)
                if label == "auto":
                    r["stream_auto_depth"] = list(fs.depth())
                fs.close()
            r["stream_fps_ratio_auto_vs_off"] = r["stream_fps_depth_auto"] / r["stream_fps_depth_off"]
            res[name] = r
            print(name, json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        dev.set_lens(0)
        dev.set_depth(0)
        dev.set_depth_auto(-1.0, 1.0)


if __name__ == "__main__":
    main()
