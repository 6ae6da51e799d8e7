"""What the map formats of a frame stream (stm_stream_maps) cost and save at 1920 x 1080 per eye, D = 64.
  - kernel time: stm_k_disp_plane under stm_prof_* (its launcher carries the scope "maps_plane") in a u8 and in a u16 stream with both
    planes -- with the profiler on a stream launches eagerly --, the median of --frames frames.  stm_k_front carries no event scope, and
    giving it one would touch the default path: it is read next to the two stm_k_disp_plane instances from the statistics of a
    rocprofv3 --kernel-trace --stats run of --profile-run (the u8 and the u16 stream alternating, 20 frames each), handed over with
    --kernel-stats FILE.csv (and --kernel-trace FILE.csv, the dispatches of the same run, for medians: the averages carry every
    stream's cold first launches);
  - bytes downloaded per frame for each format (arithmetic on the stream's geometry: the two maps or planes and the BGR frame);
  - the frame stream's frames per second through its zero-copy entry points, two frames in flight, BGR in and out, for formats f32,
    none and u8 (both planes): the median, the least and the greatest of --stream-runs (3) fresh streams of --stream-frames frames
    each, the formats in turn and the order rotating, on the synthetic pair bench.py times and on the tiled real-content bud pair.
    Two formats differ where their [least, greatest] ranges are disjoint; the file says which pairs are.
usage: python tools/maps_time.py [--frames N] [--stream-frames M] [--stream-runs R] [--kernel-stats FILE.csv] [--kernel-trace FILE.csv] [--out FILE.json]
       [--profile-run]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = (0.0, 64.0)  # lo, hi of the planes: the disparity range of D = 64 (the kernel's time does not depend on them)
FORMATS = [("f32", None), ("none", ("none",)), ("u8", ("u8", "both") + LIMITS)]


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


def stream_rate(video, p, H, W, frame, maps, n):
    """frames per second of a FrameStream over n copies of `frame`, two in flight, zero-copy entry points"""
    fs = video.FrameStream(H, W, p, maps=maps)
    try:
        run_frames(fs, frame, 8)  # eager and captured frames of both slots
        t0 = time.perf_counter()
        run_frames(fs, frame, n)
        return n / (time.perf_counter() - t0)
    finally:
        fs.close()


def kernel_rows(path):
    """the rows of a rocprofv3 kernel statistics file for stm_k_front and stm_k_disp_plane: {name: {calls, average_us, min_us, max_us}}"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if "stm_k_disp_plane" in name or "stm::stm_k_front(" in name or "stm::stm_k_front<" in name:
                out[name] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                             "max_us": float(row["MaxNs"]) / 1e3}
    return out


def kernel_trace_rows(path):
    """the same two kernels from the run's kernel trace: the statistics' averages carry the cold first launches of every stream, so
    {name: {calls, median_us, min_us}} from the dispatches themselves"""
    t = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if "stm_k_disp_plane" in name or "stm::stm_k_front(" in name or "stm::stm_k_front<" in name:
                t.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {name: {"calls": len(v), "median_us": float(np.median(v)), "min_us": float(min(v))} for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--stream-frames", type=int, default=600)
    ap.add_argument("--stream-runs", type=int, default=3, help="fresh streams per format for the stream rate")
    ap.add_argument("--kernel-stats", default=None, help="the kernel statistics CSV of a rocprofv3 run of --profile-run")
    ap.add_argument("--kernel-trace", default=None, help="the kernel trace CSV of the same run: medians in place of the statistics' averages")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    args = ap.parse_args()
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, synth, video
    stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    frames = {"synthetic": synth.sbs_frame(H, W, D, zd)[0], "real_content": synth.tiled_sbs_frame(bud[0], bud[1], H, W)}
    both = {"u8": ("u8", "both") + LIMITS, "u16": ("u16", "both") + LIMITS}
    if args.profile_run:
        for _ in range(2):
            for fmt in ("u8", "u16"):
                fs = video.FrameStream(H, W, p, maps=both[fmt])
                try:
                    run_frames(fs, frames["synthetic"], 10)
                finally:
                    fs.close()
        print("profile run done")
        return
    out_frame, maps_f32 = H * W * 3, 2 * H * W * 4
    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "frames": args.frames, "stream_frames": args.stream_frames,
           "limits": list(LIMITS),
           "download_bytes_per_frame": {"f32": out_frame + maps_f32, "none": out_frame, "u8_both": out_frame + 2 * H * W,
                                        "u8_one": out_frame + H * W, "u16_both": out_frame + 4 * H * W, "u16_one": out_frame + 2 * H * W}}
    # stm_k_disp_plane under the library's own event scopes
    us = {}
    dev.prof_enable(True)
    try:
        for fmt in ("u8", "u16"):
            fs = video.FrameStream(H, W, p, maps=both[fmt])
            try:
                t = []
                for _ in range(args.frames):
                    dev.prof_reset()
                    run_frames(fs, frames["synthetic"], 1)
                    n, ms = dev.prof_read("maps_plane")
                    assert n == 1
                    t.append(ms * 1e3)
                us[fmt + "_both"] = {"median": float(np.median(t[2:])), "min": float(min(t[2:])), "max": float(max(t[2:]))}
            finally:
                fs.close()
    finally:
        dev.prof_enable(False)
        dev.prof_reset()
    res["maps_plane_us"] = us
    if args.kernel_stats:
        res["kernel_stats_same_run"] = kernel_rows(args.kernel_stats)
    if args.kernel_trace:
        res["kernel_trace_same_run"] = kernel_trace_rows(args.kernel_trace)
    print("maps_plane_us", json.dumps(us), flush=True)
    for name, frame in frames.items():
        rates = {fmt: [] for fmt, _ in FORMATS}
        for i in range(args.stream_runs):  # a fresh stream per run, the formats in turn, the order rotating
            k = i % len(FORMATS)
            for fmt, maps in FORMATS[k:] + FORMATS[:k]:
                rates[fmt].append(stream_rate(video, p, H, W, frame, maps, args.stream_frames))
        r = {fmt: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": v} for fmt, v in rates.items()}
        r["disjoint_ranges"] = {"%s_vs_%s" % (a, b): bool(r[a]["min"] > r[b]["max"] or r[b]["min"] > r[a]["max"])
                                for a, b in (("none", "f32"), ("u8", "f32"), ("none", "u8"))}
        res["stream_frames_per_s_" + name] = r
        print(name, json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
