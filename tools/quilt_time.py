"""Cost of the quilt output (stm_set_layout) at 1920 x 1080 per view, D = 64, default parameters, stages 3.

Three layouts -- 8 views as 4 x 2 tiles in a 1920 x 1080 frame, 48 views as 8 x 6 tiles in a 3360 x 3360 frame (the Looking Glass
quilt), 2 views as 2 x 1 tiles in a 3840 x 1080 frame (a stereo pair) -- each in three forms: filter 0 (the four-neighbour sampler,
fused), filter 1 (the area average, fused: no view written) and filter 1 un-fused (stm_set_agg_variant(200): every view written by
stm_k_view_synth_all, then tiled by stm_k_quilt_area from the table), and the interlaced frame of the same size as the yardstick.
For the synthetic frame bench.py times and the tiled real-content bud pair:
  - frame time of every form, the forms alternating frame by frame in one process, HIP events around each frame (after a warm-up),
    median and mean;
  - the render kernels of every form from stm_prof_read (`synth_quilt`; un-fused: `view_synth` + `quilt`; interlaced: `synth_mux`),
    alternating, one profiled frame at a time;
  - for the fused area filter, from the geometry: the view pixels it renders (every block's footprint) against the ideal of one
    render per view pixel, the bytes those renders ask for and the bytes the un-fused form moves, over the kernel time.
usage: python tools/quilt_time.py [--frames N] [--warmup W] [--out FILE.json] [--profile-run]
--profile-run: five frames of every form and nothing else (for rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYOUTS = [("4x2_1920x1080", 8, 4, 2, 1080, 1920), ("8x6_3360x3360", 48, 8, 6, 3360, 3360), ("2x1_3840x1080", 2, 2, 1, 1080, 3840)]
FORMS = ["interlaced", "filter0", "filter1", "filter1_unfused"]
LDS_LIMIT = 32 * 1024


def cdiv(a, b):
    return (a + b - 1) // b


def staged_block(Hin, Win, th, tw, limit=LDS_LIMIT):
    """the block of stm_k_quilt_area as launch_quilt_src sizes it: (BW, BH, fw_max, fh_max, bytes), or None (the per-pixel form)"""
    BW, BH = 32, 16
    while True:
        fw, fh = min(Win, cdiv(BW * Win, tw) + 1), min(Hin, cdiv(BH * Hin, th) + 1)
        nbytes = 4 * (fw * fh + fh * BW * 3)
        if nbytes <= limit:
            return BW, BH, fw, fh, nbytes
        if BH > 1 and (fh >= fw or BW == 1):
            BH //= 2
        elif BW > 1:
            BW //= 2
        else:
            return None


def renders_per_view(Hin, Win, th, tw, BW, BH):
    """view pixels one tile's blocks render: the sum of every block's footprint"""
    def spans(t, n, B):
        return sum(((min(u0 + B, t)) * n - 1) // t - (u0 * n) // t + 1 for u0 in range(0, t, B))
    return spans(tw, Win, BW) * spans(th, Hin, BH)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    args = ap.parse_args()
    import torch
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, synth
    lib = stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    frames = {"synthetic": synth.sbs_frame(H, W, D, zd)[0], "real_content": synth.tiled_sbs_frame(bud[0], bud[1], H, W)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    outs = {name: torch.zeros(Ho, Wo, 3, dtype=torch.uint8, device="cuda") for name, _, _, _, Ho, Wo in LAYOUTS}
    params = {name: dev.FrameParams(num_disp=D, zero_disp=zd, num_views=N) for name, N, _, _, _, _ in LAYOUTS}
    configs = [(lay, form) for lay in LAYOUTS for form in FORMS]

    def frame(d_sbs, cfg):
        (name, N, tx, ty, Ho, Wo), form = cfg
        if form == "interlaced":
            dev.set_layout(0)
        else:
            dev.set_layout(1, tx, ty, 3, 0 if form == "filter0" else 1)
        lib.stm_set_agg_variant(200 if form == "filter1_unfused" else 0)
        dev.d_adcensus_stm(d_sbs, dl, dr, outs[name], params[name], stages=3)

    def rot(i):
        k = i % len(configs)
        return configs[k:] + configs[:k]

    def key(cfg):
        return cfg[0][0] + "_" + cfg[1]

    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "stages": 3, "order": 3, "frames": args.frames, "warmup": args.warmup,
           "layouts": [list(x) for x in LAYOUTS]}
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
            for cfg in configs:  # the two area forms give the same bytes
                frame(d_sbs, cfg)
                torch.cuda.synchronize()
                keep[key(cfg)] = outs[cfg[0][0]].cpu().numpy()
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
            nprof = 12
            tot = {key(cfg): {} for cfg in configs}
            dev.prof_enable(True)
            for i in range(nprof):
                for cfg in rot(i):
                    dev.prof_reset()
                    frame(d_sbs, cfg)
                    torch.cuda.synchronize()
                    names = {"interlaced": ["synth_mux"], "filter1_unfused": ["view_synth", "quilt"]}.get(cfg[1], ["synth_quilt"])
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
            for lay in LAYOUTS:
                name, N, tx, ty, Ho, Wo = lay
                tw, th = Wo // tx, Ho // ty
                assert np.array_equal(keep[name + "_filter1"], keep[name + "_filter1_unfused"]), name
                blk = staged_block(H, W, th, tw)
                BW, BH, fw, fh, nbytes = blk
                renders = N * renders_per_view(H, W, th, tw, BW, BH)
                ideal = N * H * W
                # a render reads its pixel's five float maps and one tap of each image (3 bytes each); the un-fused form writes every
                # interior view once (3 bytes a pixel) and reads every view once (the footprints of a tile partition the view)
                fused_bytes = renders * (5 * 4 + 2 * 3) + Ho * Wo * 3
                unfused_bytes = max(N - 2, 0) * H * W * (5 * 4 + 2 * 3 + 3) + ideal * 3 + Ho * Wo * 3
                t_f, t_u = r[name + "_filter1_render_ms"], r[name + "_filter1_unfused_render_ms"]
                r[name + "_geometry"] = {"tile": [th, tw], "block": [BH, BW], "footprint_max": [fh, fw], "lds_bytes": nbytes,
                                         "renders": renders, "ideal_renders": ideal, "renders_per_view_pixel": renders / ideal,
                                         "renders_per_output_pixel": renders / (N * th * tw), "ideal_renders_per_output_pixel": ideal / (N * th * tw),
                                         "fused_bytes_requested": fused_bytes, "fused_GB_per_s": fused_bytes / t_f / 1e6,
                                         "unfused_bytes": unfused_bytes, "unfused_GB_per_s": unfused_bytes / t_u / 1e6,
                                         "fused_over_unfused_render_time": t_f / t_u}
            res[cname] = r
            print(cname, json.dumps(r), flush=True)
        if args.out and not args.profile_run:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    finally:
        dev.set_layout(0)
        lib.stm_set_agg_variant(0)


if __name__ == "__main__":
    main()
