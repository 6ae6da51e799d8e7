"""Cost of the reduced-resolution frame's front (the split, the two reductions, the reduced pair's pixel formats and census words)
as one kernel, stm_k_front_low, against the chain of six launches it replaces, and the rate of a frame stream that runs the
reduced frame.

Part 1 (default): 1920 x 1080 eyes matched at 960 x 540, D = 64, default parameters, the synthetic frame bench.py times and the
tiled real-content bud pair.  stm_set_agg_variant(600) -- the chain, which is the parent commit's front -- and the default
alternate frame by frame in one process:
  - frame time of stm_d_adcensus_stm_2s, HIP events around each frame (after a warm-up), median and mean;
  - the front alone from the library's own events (stm_prof_read("reduced_front"): the scope spans the one launch or the three
    image-sized launches of the chain; the chain's pack and census launches run inside the match and are read as the difference
    of the two frame times).
Part 2 (--stream): frames/s of a zero-copy FrameStream, 3840 x 2160 eyes matched at 1920 x 1080 with D = 128 and disp_scale 0.5
(plain, with 0x1000, and from NV12 input) against the full-resolution stream at D = 256; the kinds alternate, several streams each,
the median is reported.
usage: python tools/reduced_time.py [--frames N] [--warmup W] [--out FILE.json] [--profile-run]
       python tools/reduced_time.py --stream [--frames N] [--rounds R] [--out FILE.json]
--profile-run: only a few frames of each kind (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = (600, 0)  # the chain of launches (the parent commit's front), the fused kernel
KEYS = {600: "chain", 0: "fused"}


def front(args):
    import torch
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, synth
    lib = stm_amd.lib()
    H, W, h, w, D, zd = 1080, 1920, 540, 960, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    frames = {"synthetic": synth.sbs_frame(H, W, D, zd)[0], "real_content": synth.tiled_sbs_frame(bud[0], bud[1], H, W)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")

    def frame(d_sbs, variant):
        lib.stm_set_agg_variant(variant)
        dev.d_adcensus_stm_2s(d_sbs, dl, dr, out, p, h, w, 0.5, stages=3)

    try:
        if args.profile_run:
            for sbs in frames.values():
                d_sbs = torch.from_numpy(sbs).cuda()
                for v in VARIANTS * 5:
                    frame(d_sbs, v)
                torch.cuda.synchronize()
            print("profile run done")
            return None
        res = {"shape": [H, W], "match_shape": [h, w], "num_disp": D, "zero_disp": zd, "frames": args.frames, "warmup": args.warmup}
        for name, sbs in frames.items():
            d_sbs = torch.from_numpy(sbs).cuda()
            maps = {}
            for v in VARIANTS:
                frame(d_sbs, v)
                torch.cuda.synchronize()
                maps[v] = (dl.cpu().numpy().copy(), dr.cpu().numpy().copy(), out.cpu().numpy().copy())
            r = {"outputs_equal": bool(all(np.array_equal(a, b) for a, b in zip(maps[600], maps[0])))}
            for _ in range(args.warmup):
                for v in VARIANTS:
                    frame(d_sbs, v)
            torch.cuda.synchronize()
            ms = {v: [] for v in VARIANTS}
            for i in range(args.frames):
                for v in (VARIANTS if i % 2 == 0 else VARIANTS[::-1]):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    frame(d_sbs, v)
                    e1.record()
                    e1.synchronize()
                    ms[v].append(e0.elapsed_time(e1))
            for v in VARIANTS:
                a = np.array(ms[v])
                r["frame_%s_ms_median" % KEYS[v]] = float(np.median(a))
                r["frame_%s_ms_mean" % KEYS[v]] = float(a.mean())
            r["frame_delta_ms_median"] = r["frame_fused_ms_median"] - r["frame_chain_ms_median"]
            r["frame_delta_share"] = r["frame_delta_ms_median"] / r["frame_chain_ms_median"]
            # the front from the library's own events, one profiled frame at a time, the two forms alternating
            t = {v: [] for v in VARIANTS}
            dev.prof_enable(True)
            for i in range(args.frames):
                for v in (VARIANTS if i % 2 == 0 else VARIANTS[::-1]):
                    dev.prof_reset()
                    frame(d_sbs, v)
                    torch.cuda.synchronize()
                    n, tf = dev.prof_read("reduced_front")
                    assert n == 1, (v, n)
                    t[v].append(tf)
            dev.prof_enable(False)
            dev.prof_reset()
            for v in VARIANTS:
                r["front_%s_ms_median" % KEYS[v]] = float(np.median(np.array(t[v])))
            r["front_chain_note"] = "demux + 2 scale launches; the chain's 2 pack + 1 census launches run inside the match"
            res[name] = r
            print(name, json.dumps(r), flush=True)
        return res
    finally:
        lib.stm_set_agg_variant(0)


def stream_rate(fs, frame, n):
    """frames/s of n zero-copy frames through fs (two in flight), after four frames that size, capture and first replay"""
    def run(k):
        pending = 0
        for _ in range(k):
            if pending == 2:
                fs.collect_view()
                pending -= 1
            fs.input_buffer()[...] = frame
            fs.submit_inplace()
            pending += 1
        while pending:
            fs.collect_view()
            pending -= 1
    run(4)
    t0 = time.perf_counter()
    run(n)
    return n / (time.perf_counter() - t0)


def stream(args):
    import stm_amd
    from stm_amd import device_api as dev, synth, video
    stm_amd.lib()
    H, W, h, w = 2160, 3840, 1080, 1920
    sbs = synth.sbs_frame(H, W, 256, 128)[0]
    # an NV12 frame of the same size: the content does not matter for the rate, the bytes moved and converted do
    nv = np.ascontiguousarray(np.concatenate([sbs[..., 1], sbs[::2, :, 0]], axis=0))
    full, low = dev.FrameParams(num_disp=256, zero_disp=128), dev.FrameParams(num_disp=128, zero_disp=64)
    kinds = {"full_d256": dict(params=full), "match_d128": dict(params=low, match=(h, w, 0.5)),
             "match_d128_guided": dict(params=low, match=(h, w, 0.5), stages=3 | 0x1000),
             "match_d128_nv12": dict(params=low, match=(h, w, 0.5), input_format="nv12")}
    rates = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, kw in kinds.items():
            kw = dict(kw)
            fs = video.FrameStream(H, W, kw.pop("params"), **kw)
            rates[k].append(stream_rate(fs, nv if kw.get("input_format") == "nv12" else sbs, args.frames))
            fs.close()
            print(k, "%.2f frames/s" % rates[k][-1], flush=True)
    res = {"shape": [H, W], "match_shape": [h, w], "frames": args.frames, "rounds": args.rounds}
    for k, v in rates.items():
        res[k] = {"fps_median": float(np.median(v)), "fps_all": [float(x) for x in v]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--stream", action="store_true")
    args = ap.parse_args()
    res = stream(args) if args.stream else front(args)
    if res is not None:
        print(json.dumps(res))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
