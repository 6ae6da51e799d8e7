"""What image-plus-depth input of a frame stream (stm_stream_input_depth) costs at 1920 x 1080, on the tiled real-content bud pair:
the left image with its own plane -- the left map a stereo stream computes on the pair -- against the stereo stream on the same pair.
  - kernel time: stm_k_eye for u8, u16 and f32 planes next to stm_k_front, from the statistics and the dispatches of ONE rocprofv3
    --kernel-trace --stats run of --profile-run (a stereo stream, then a depth stream per format, 100 frames each), handed over with
    --kernel-stats FILE.csv and --kernel-trace FILE.csv (medians: the statistics' averages carry every stream's cold first launches);
  - bytes a frame uploads and downloads, for both streams (arithmetic on the stream's geometry);
  - frames per second through the zero-copy entry points, two frames in flight: the median, the least and the greatest of
    --stream-runs (3) fresh streams of --stream-frames frames each, the two kinds in turn and the order alternating.
usage: python tools/depth_input_time.py [--stream-frames M] [--stream-runs R] [--kernel-stats FILE.csv] [--kernel-trace FILE.csv]
       [--out FILE.json] [--profile-run]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = (-32.0, 32.0)  # lo, hi of the planes: the disparity range of D = 64, zero_disp = 32
KERNELS = ("stm_k_eye", "stm::stm_k_front(", "stm::stm_k_front<")


def quantise(d, maxcode):
    """stm_stream_maps' plane of a float map (include/stm_hip.h), in float32"""
    f = np.float32
    k = f(float(maxcode) / (float(f(LIMITS[1])) - float(f(LIMITS[0]))))
    t = (d.astype(f) - f(LIMITS[0])) * k
    t = np.minimum(np.maximum(t, f(0)), f(maxcode))
    return (t + f(0.5)).astype(np.uint8 if maxcode == 255 else np.uint16)


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


def stream_rate(make, frame, n):
    fs = make()
    try:
        run_frames(fs, frame, 8)  # eager and captured frames of both slots
        t0 = time.perf_counter()
        run_frames(fs, frame, n)
        return n / (time.perf_counter() - t0)
    finally:
        fs.close()


def kernel_rows(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if any(k in row["Name"] for k in KERNELS):
                out[row["Name"]] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                                    "max_us": float(row["MaxNs"]) / 1e3}
    return out


def kernel_trace_rows(path):
    t = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if any(k in row["Kernel_Name"] for k in KERNELS):
                t.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {name: {"calls": len(v), "median_us": float(np.median(v)), "min_us": float(min(v))} for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream-frames", type=int, default=3000)
    ap.add_argument("--stream-runs", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    args = ap.parse_args()
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, synth, video
    stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    sbs = synth.tiled_sbs_frame(bud[0], bud[1], H, W)
    left = np.ascontiguousarray(sbs[:, :W])

    def stereo():
        return video.FrameStream(H, W, p)

    def depth(fmt):
        return video.FrameStream(H, W, p, depth_input=(fmt,) + LIMITS + (1, 0.5))
    fs = stereo()
    try:  # the pair's own left map: what the planes hold
        run_frames(fs, sbs, 100 if args.profile_run else 1)
        fs.submit(sbs)
        dl = np.array(fs.collect()[1])
    finally:
        fs.close()
    planes = {"u8": quantise(dl, 255), "u16": quantise(dl, 65535), "f32": dl}
    frames = {}
    for fmt, plane in planes.items():
        fs = depth(fmt)
        frames[fmt] = fs.pack_depth_frame(left, plane)
        fs.close()
    if args.profile_run:
        for fmt in ("u8", "u16", "f32"):
            fs = depth(fmt)
            try:
                run_frames(fs, frames[fmt], 100)
            finally:
                fs.close()
        print("profile run done")
        return
    out_bytes, maps = H * W * 3, 2 * H * W * 4
    res = {"shape": [H, W], "content": "tiled bud pair; the depth stream takes its left image and the pair's own left map as a plane",
           "limits": list(LIMITS), "fill": 1, "gate": 0.5, "stream_frames": args.stream_frames,
           "bytes_per_frame": {"stereo": {"upload": int(sbs.nbytes), "download": out_bytes + maps},
                               "depth_u8": {"upload": int(frames["u8"].nbytes), "download": out_bytes + maps},
                               "depth_u16": {"upload": int(frames["u16"].nbytes), "download": out_bytes + maps},
                               "depth_f32": {"upload": int(frames["f32"].nbytes), "download": out_bytes + maps}}}
    if args.kernel_stats:
        res["kernel_stats_same_run"] = kernel_rows(args.kernel_stats)
    if args.kernel_trace:
        res["kernel_trace_same_run"] = kernel_trace_rows(args.kernel_trace)
    kinds = [("depth_u8", lambda: depth("u8"), frames["u8"]), ("stereo", stereo, sbs)]
    rates = {k: [] for k, _, _ in kinds}
    for i in range(args.stream_runs):
        for k, make, frame in (kinds if i % 2 == 0 else kinds[::-1]):
            rates[k].append(stream_rate(make, frame, args.stream_frames))
    r = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": v} for k, v in rates.items()}
    for k in r:  # what the link carries at that rate, both directions
        b = res["bytes_per_frame"][k]
        r[k]["upload_GB_per_s"] = r[k]["median"] * b["upload"] / 1e9
        r[k]["download_GB_per_s"] = r[k]["median"] * b["download"] / 1e9
    res["stream_frames_per_s"] = r
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
