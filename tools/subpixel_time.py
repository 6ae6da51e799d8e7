"""Cost of the sub-pixel enhancement (stages bit 0x200) at 1920 x 1080, D = 64, default parameters.

For the synthetic frame bench.py times and the tiled real-content bud pair:
  - frame time of stages 3 against 3 | 0x200, the two alternating frame by frame in one process, HIP events around each frame
    (after a warm-up), median and mean;
  - the `subpixel` kernel and the `bilateral` kernel from stm_prof_read (a separate, profiled loop);
  - the bytes the kernel moves: the 128-byte lines of V2 (the PQ input of the last horizontal pass) that the windows of the
    eligible pixels touch, computed from the arms and the post-voting maps (each line counted once: what HBM / MALL must
    deliver at the least), the bytes the lanes request (3 x 16 B per window group), and 3 x 4 B per pixel for comparison;
  - the two bilateral kernels on a sub-pixel map (the per-stage filter through the integer-map kernel, variant 500, which
    checks each tile and falls back, against the general kernel): the choice the frame pipeline makes after 0x200.
usage: python tools/subpixel_time.py [--frames N] [--warmup W] [--out FILE.json] [--profile-run]
--profile-run: only a few frames with 0x200 (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUB = 0x200


def v2_traffic(orc, L, R, wl, wr, p, H, W):
    """V2 bytes of the kernel for both views: (distinct 128-B lines x 128, requested bytes, 3 x 4 B per eligible pixel)"""
    D, zd = p.num_disp, p.zero_disp
    G, NC = (W + 3) // 4, (D + 15) // 16
    lines = req = naive = 0
    for img, disp in ((L, wl), (R, wr)):
        cross = orc.cross_arms(img, p.ucd, p.lcd, p.usd, p.lsd)
        x = np.arange(W)[None, :].repeat(H, 0)
        y = np.arange(H)[:, None].repeat(W, 1)
        a = x - cross[2].astype(np.int64)
        b = x + cross[3].astype(np.int64)
        ok = (disp == np.floor(disp)) & (disp + zd >= 1) & (disp + zd <= D - 2) & (b > a)
        d = (disp[ok] + zd).astype(np.int64)
        g0, g1, yy = a[ok] >> 2, (b[ok] - 1) >> 2, y[ok]
        naive += 12 * int(ok.sum())
        req += int(3 * 16 * (g1 - g0 + 1).sum())
        # a 256-B record [c][y][g] holds 16 hypotheses x 16 B: hypotheses 0-7 in its first 128-B line, 8-15 in the second
        mark = np.zeros((H, NC * 2, G + 1), np.int32)
        for k in (d - 1, d, d + 1):
            seg = (k >> 4) * 2 + ((k & 15) >> 3)
            np.add.at(mark, (yy, seg, g0), 1)
            np.add.at(mark, (yy, seg, g1 + 1), -1)
        lines += int((np.cumsum(mark, axis=2)[:, :, :G] > 0).sum())
    return lines * 128, req, naive


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
    lib = stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    frames = {"synthetic": synth.sbs_frame(H, W, D, zd)[0], "real_content": synth.tiled_sbs_frame(bud[0], bud[1], H, W)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    if args.profile_run:
        d_sbs = torch.from_numpy(frames["synthetic"]).cuda()
        for st in (3, 3 | SUB) * 5:
            dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
        torch.cuda.synchronize()
        print("profile run done")
        return
    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "frames": args.frames, "warmup": args.warmup}
    for name, sbs in frames.items():
        d_sbs = torch.from_numpy(sbs).cuda()
        for _ in range(args.warmup):
            for st in (3, 3 | SUB):
                dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
        torch.cuda.synchronize()
        ms = {3: [], 3 | SUB: []}
        for i in range(args.frames):
            for st in ((3, 3 | SUB) if i % 2 == 0 else (3 | SUB, 3)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
                e1.record()
                e1.synchronize()
                ms[st].append(e0.elapsed_time(e1))
        r = {}
        for st, key in ((3, "stages3"), (3 | SUB, "stages3_subpixel")):
            a = np.array(ms[st])
            r[key + "_ms_median"] = float(np.median(a))
            r[key + "_ms_mean"] = float(a.mean())
        r["frame_delta_ms_median"] = r["stages3_subpixel_ms_median"] - r["stages3_ms_median"]
        # kernel times from the library's own events
        for st, key in ((3, "stages3"), (3 | SUB, "stages3_subpixel")):
            dev.prof_reset()
            dev.prof_enable(True)
            for _ in range(20):
                dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=st)
            torch.cuda.synchronize()
            dev.prof_enable(False)
            for k in ("subpixel", "bilateral", "irv"):
                n, t = dev.prof_read(k)
                if n:
                    r["%s_%s_kernel_ms" % (key, k)] = t / n
        # bytes: the post-voting maps (stages 2 without the step, before the filter, come from the oracle's DCC + IRV on
        # the GPU's WTA maps -- bit-identical to the frame's own)
        from oracle import pyoracle as orc
        dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=1)
        torch.cuda.synchronize()
        wl, wr = dl.cpu().numpy(), dr.cpu().numpy()
        L, R = orc.demux_sbs(sbs, W)
        xl, xr = orc.cross_arms(L, p.ucd, p.lcd, p.usd, p.lsd), orc.cross_arms(R, p.ucd, p.lcd, p.usd, p.lsd)
        ol, orr = orc.dr_dcc(wl, wr)
        wl, _ = orc.dr_irv(wl, ol, xl, p.thresh_s, p.thresh_h, D, zd, p.usd, 5, device_flavour=True)
        wr, _ = orc.dr_irv(wr, orr, xr, p.thresh_s, p.thresh_h, D, zd, p.usd, 5, device_flavour=True)
        lines_b, req_b, naive_b = v2_traffic(orc, L, R, wl, wr, p, H, W)
        r["v2_distinct_line_bytes"] = lines_b
        r["v2_requested_bytes"] = req_b
        r["three_costs_bytes"] = naive_b
        r["eligible_fraction"] = float(np.mean([((m == np.floor(m)) & (m + zd >= 1) & (m + zd <= D - 2)).mean() for m in (wl, wr)]))
        res[name] = r
        print(name, json.dumps(r), flush=True)
    # the bilateral filter on a sub-pixel map: integer-map kernel (tile check + fallback) vs the general kernel
    d_sbs = torch.from_numpy(frames["synthetic"]).cuda()
    dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=1 | SUB)
    torch.cuda.synchronize()
    src = dl.clone()
    bil = {}
    for variant, key in ((500, "integer_map_kernel"), (0, "general_kernel")):
        lib.stm_set_agg_variant(variant)
        img = src.clone()
        for _ in range(3):
            img.copy_(src)
            lib.stm_d_filter_bilateral_1(dev._p(img), 7, 5.0, 10.0, H, W, D)
        torch.cuda.synchronize()
        dev.prof_reset()
        dev.prof_enable(True)
        for _ in range(20):
            img.copy_(src)
            dev._use_current_stream()
            lib.stm_d_filter_bilateral_1(dev._p(img), 7, 5.0, 10.0, H, W, D)
        torch.cuda.synchronize()
        dev.prof_enable(False)
        n, t = dev.prof_read("bilateral")
        bil[key + "_ms"] = t / max(n, 1)
    lib.stm_set_agg_variant(0)
    res["bilateral_on_subpixel_map_one_view"] = bil
    print("bilateral", json.dumps(bil), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
