"""Cost of the NV12 output (stm_set_output) at 1920 x 1080 per view, D = 64, default parameters, stages 3.

The three layouts of tools/quilt_time.py -- 8 views as 4 x 2 tiles in 1920 x 1080, 48 views as 8 x 6 tiles in 3360 x 3360, 2 views
as 2 x 1 tiles in 3840 x 1080 -- with both filters, each in four forms: the BGR quilt (the yardstick), the NV12 quilt fused (the
conversion inside the kernel that renders), and both again under stm_set_agg_variant(200), the un-fused forms (every view written,
tiled into a BGR quilt; for NV12 that quilt lies in the workspace and stm_k_mux_nv12 converts it).  For the synthetic frame bench.py
times and the tiled real-content bud pair:
  - frame time of every form, the forms alternating frame by frame in one process, HIP events around each frame (after a warm-up),
    median and mean;
  - the render kernels of every form from stm_prof_read (`synth_quilt`; un-fused: `view_synth` + `quilt` + `mux_nv12`), alternating,
    one profiled frame at a time.
--stream: instead, the rate of a frame stream with its upload and download, a BGR quilt stream against an NV12 quilt stream (filter
1) at 4 x 2 and 8 x 6, alternating `--pairs` times, `--frames` frames each; medians, ranges, and whether the ranges are disjoint.
usage: python tools/nv12out_time.py [--frames N] [--warmup W] [--out FILE.json] [--stream [--pairs P]] [--profile-run]
--profile-run: five frames of every form and nothing else (for rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYOUTS = [("4x2_1920x1080", 8, 4, 2, 1080, 1920), ("8x6_3360x3360", 48, 8, 6, 3360, 3360), ("2x1_3840x1080", 2, 2, 1, 1080, 3840)]
FORMS = ["bgr", "nv12", "bgr_unfused", "nv12_unfused"]
MATRIX = 1


def stream_rates(args, frames_in, res):
    from stm_amd import device_api as dev, video
    H, W, D, zd = 1080, 1920, 64, 32
    for name, N, tx, ty, Ho, Wo in LAYOUTS[:2]:
        p = dev.FrameParams(num_disp=D, zero_disp=zd, num_views=N)
        fps = {"bgr": [], "nv12": []}
        for pair in range(args.pairs):
            for form in (("bgr", "nv12") if pair % 2 == 0 else ("nv12", "bgr")):
                fs = video.FrameStream(H, W, p, Ho, Wo, layout=(1, tx, ty, 3, 1), output=(1, MATRIX) if form == "nv12" else None)
                try:
                    n = args.warmup + args.frames
                    t0 = None
                    for k in range(n + 2):
                        if k >= 2:
                            assert fs.collect_view() is not None
                            if k - 2 == args.warmup - 1:
                                t0 = time.perf_counter()
                        if k < n:
                            fs.submit(frames_in)
                    fps[form].append(args.frames / (time.perf_counter() - t0))
                finally:
                    fs.close()
        r = {}
        for form, a in fps.items():
            r[form + "_fps"] = a
            r[form + "_fps_median"] = float(np.median(a))
            r[form + "_fps_range"] = [float(min(a)), float(max(a))]
        r["ranges_disjoint"] = bool(min(fps["nv12"]) > max(fps["bgr"]) or min(fps["bgr"]) > max(fps["nv12"]))
        r["bytes_per_frame"] = {"bgr": Ho * Wo * 3, "nv12": Ho * Wo * 3 // 2}
        res["stream_" + name] = r
        print(name, json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--profile-run", action="store_true")
    args = ap.parse_args()
    import torch
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, synth
    lib = stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "stages": 3, "order": 3, "matrix": MATRIX, "frames": args.frames,
           "warmup": args.warmup, "layouts": [list(x) for x in LAYOUTS]}
    if args.stream:
        res["pairs"] = args.pairs
        stream_rates(args, synth.sbs_frame(H, W, D, zd)[0], res)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    frames = {"synthetic": synth.sbs_frame(H, W, D, zd)[0], "real_content": synth.tiled_sbs_frame(bud[0], bud[1], H, W)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    bgr = {name: torch.zeros(Ho, Wo, 3, dtype=torch.uint8, device="cuda") for name, _, _, _, Ho, Wo in LAYOUTS}
    nv12 = {name: torch.zeros(Ho * 3 // 2, Wo, dtype=torch.uint8, device="cuda") for name, _, _, _, Ho, Wo in LAYOUTS}
    params = {name: dev.FrameParams(num_disp=D, zero_disp=zd, num_views=N) for name, N, _, _, _, _ in LAYOUTS}
    configs = [(lay, filt, form) for lay in LAYOUTS for filt in (0, 1) for form in FORMS]

    def frame(d_sbs, cfg):
        (name, N, tx, ty, Ho, Wo), filt, form = cfg
        dev.set_layout(1, tx, ty, 3, filt)
        lib.stm_set_agg_variant(200 if form.endswith("unfused") else 0)
        if form.startswith("nv12"):
            dev.set_output(1, MATRIX)
            dev.d_adcensus_stm(d_sbs, dl, dr, nv12[name], params[name], stages=3)
        else:
            dev.set_output(0)
            dev.d_adcensus_stm(d_sbs, dl, dr, bgr[name], params[name], stages=3)

    def rot(i):
        k = i % len(configs)
        return configs[k:] + configs[:k]

    def key(cfg):
        return "%s_filter%d_%s" % (cfg[0][0], cfg[1], cfg[2])

    try:
        for cname, sbs in frames.items():
            d_sbs = torch.from_numpy(sbs).cuda()
            if args.profile_run:
                for _ in range(5):
                    for cfg in configs:
                        frame(d_sbs, cfg)
                torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                for cfg in configs:
                    frame(d_sbs, cfg)
            torch.cuda.synchronize()
            keep = {}
            for cfg in configs:  # the fused and the un-fused form give the same bytes
                frame(d_sbs, cfg)
                torch.cuda.synchronize()
                keep[key(cfg)] = (nv12 if cfg[2].startswith("nv12") else bgr)[cfg[0][0]].cpu().numpy()
            for (name, *_), filt, _ in configs:
                k = "%s_filter%d_" % (name, filt)
                assert np.array_equal(keep[k + "nv12"], keep[k + "nv12_unfused"]) and np.array_equal(keep[k + "bgr"], keep[k + "bgr_unfused"]), k
            ms = {key(cfg): [] for cfg in configs}
            for i in range(args.frames):
                for cfg in rot(i):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    frame(d_sbs, cfg)
                    e1.record()
                    e1.synchronize()
                    ms[key(cfg)].append(e0.elapsed_time(e1))
            r = {}
            for cfg in configs:
                a = np.array(ms[key(cfg)])
                r[key(cfg) + "_frame_ms_median"] = float(np.median(a))
                r[key(cfg) + "_frame_ms_mean"] = float(a.mean())
            nprof = 8
            tot = {key(cfg): {} for cfg in configs}
            dev.prof_enable(True)
            for i in range(nprof):
                for cfg in rot(i):
                    dev.prof_reset()
                    frame(d_sbs, cfg)
                    torch.cuda.synchronize()
                    names = ["view_synth", "quilt"] if cfg[2].endswith("unfused") else ["synth_quilt"]
                    if cfg[2] == "nv12_unfused":
                        names.append("mux_nv12")
                    for kn in names:
                        n, t = dev.prof_read(kn)
                        assert n == (0 if kn == "view_synth" and cfg[0][1] < 3 else 1), (key(cfg), kn, n)
                        tot[key(cfg)][kn] = tot[key(cfg)].get(kn, 0.0) + t
            dev.prof_enable(False)
            dev.prof_reset()
            for cfg in configs:
                for kn, t in tot[key(cfg)].items():
                    r[key(cfg) + "_" + kn + "_ms"] = t / nprof
                r[key(cfg) + "_render_ms"] = sum(tot[key(cfg)].values()) / nprof
            res[cname] = r
            print(cname, json.dumps(r), flush=True)
        if args.out and not args.profile_run:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        dev.set_output(0)
        dev.set_layout(0)
        lib.stm_set_agg_variant(0)


if __name__ == "__main__":
    main()
