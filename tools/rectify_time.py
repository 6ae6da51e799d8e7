"""Cost of the rectification of a frame stream (stm_stream_rectify) at 1920 x 1080, D = 64, default parameters, stages 3, on the
tiled real-content bud pair, for BGR and NV12 input and two records per eye: the identity, and a roll of 1 degree with k1 = -0.1.
  - kernel time: `rectify` (stm_k_rectify) next to `align_frame` (the yardstick: the same traffic class, both eyes read and one
    side-by-side frame written) and `front` (stm_k_front) in the same frames of a stream that also has a manual alignment, from
    stm_prof_read (profiling keeps the stream's frames eager), mean and least of --prof-frames frames;
  - frame time: a stream with the setting off and one with it on, both alive, taking turns in blocks of --block pipelined frames
    through the zero-copy entry points (two frames in flight), wall clock per frame, median over --blocks blocks each.
usage: python tools/rectify_time.py [--prof-frames N] [--blocks B] [--block K] [--out FILE.json]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("rectify", "align_frame", "front")


def run_frames(fs, frame, count):
    pending = 0
    for _ in range(count):
        if pending == 2:
            fs.collect_view()
            pending -= 1
        fs.input_buffer()[...] = frame
        assert fs.submit_inplace() >= 0
        pending += 1
    while pending:
        fs.collect_view()
        pending -= 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prof-frames", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--block", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, rectify, synth, video
    stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    sbs = synth.tiled_sbs_frame(bud[0], bud[1], H, W)
    y, uv = synth.bgr_to_nv12(sbs, 0)
    inputs = {"bgr": ({}, sbs), "nv12": (dict(input_format="nv12"), np.ascontiguousarray(np.concatenate([y, uv], axis=0)))}
    a = math.radians(1.0)
    K = np.array([[1.0 * W, 0.0, (W - 1) / 2.0], [0.0, 1.0 * W, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    roll = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    records = {"identity": rectify.identity(), "roll_1deg_k1_-0.1": rectify.record(K, [-0.1], roll, K)}
    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "stages": 3, "border": 0, "prof_frames": args.prof_frames, "blocks": args.blocks,
           "block": args.block, "bytes_read_and_written": 4 * H * W * 3}
    for fmt, (kw, frame) in inputs.items():
        for rname, rec in records.items():
            r = {}
            dev.prof_enable(True)
            fs = video.FrameStream(H, W, p, rectify=(rec, rec, 0), align=(0.5, 0.0, 0.0), **kw)
            try:
                run_frames(fs, frame, 2)  # (not timed: both slots' first frames)
                t = {k: [] for k in KERNELS}
                for _ in range(args.prof_frames):
                    dev.prof_reset()
                    run_frames(fs, frame, 1)
                    for k in KERNELS:
                        n, ms = dev.prof_read(k)
                        assert n == 1, (k, n)
                        t[k].append(ms)
            finally:
                fs.close()
                dev.prof_enable(False)
                dev.prof_reset()
            for k in KERNELS:
                r[k + "_us_mean"] = 1e3 * float(np.mean(t[k]))
                r[k + "_us_min"] = 1e3 * float(min(t[k]))
            r["rectify_vs_align_frame"] = r["rectify_us_mean"] / r["align_frame_us_mean"]
            off, on = video.FrameStream(H, W, p, **kw), video.FrameStream(H, W, p, rectify=(rec, rec, 0), **kw)
            try:
                ms = {"off": [], "on": []}
                for fs in (off, on):
                    run_frames(fs, frame, 8)  # eager and captured frames of both slots
                for i in range(args.blocks):
                    for name, fs in ((("off", off), ("on", on)) if i % 2 == 0 else (("on", on), ("off", off))):
                        t0 = time.perf_counter()
                        run_frames(fs, frame, args.block)
                        ms[name].append(1e3 * (time.perf_counter() - t0) / args.block)
            finally:
                off.close()
                on.close()
            for name in ("off", "on"):
                r["frame_ms_median_" + name] = float(np.median(ms[name]))
                r["frame_ms_min_" + name] = float(min(ms[name]))
                r["frame_ms_max_" + name] = float(max(ms[name]))
            r["frame_delta_ms_median"] = r["frame_ms_median_on"] - r["frame_ms_median_off"]
            res["%s_%s" % (fmt, rname)] = r
            print(fmt, rname, json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
