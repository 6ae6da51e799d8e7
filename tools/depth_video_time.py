"""What packed 2D-plus-depth video input of a frame stream (stm_stream_input_packed_depth) costs at 1920 x 1080, on the tiled
real-content bud pair: its left image with the pair's own left map as the depth picture.  The procedure of tools/depth_input_time.py.
  - kernel time: stm_k_eye_video in four forms (NV12 side by side full; NV12 half width, linear and Catmull-Rom image filter, dfilter
    1; BGR side by side full) next to stm_k_eye<2> (an existing u8 depth stream) and stm_k_front_pack of the same format and packing
    (packed stereo streams, run first), from the dispatches of ONE rocprofv3 --kernel-trace --stats run of --profile-run, handed over with
    --kernel-trace FILE.csv.  Each stream's first --discard (150) dispatches are dropped; the median and the minimum of the rest.
    --in-flight 1 (the default) keeps one frame in flight during that run, so that a dispatch does not share the chip with the other
    slot's tail; with 2 the light streams' dispatches overlap it and their durations measure the sharing;
  - bytes a frame uploads and downloads (arithmetic on the stream's geometry);
  - frames per second through the zero-copy entry points, two frames in flight: the median, the least and the greatest of
    --stream-runs (3) fresh streams of --stream-frames frames each, the kinds in turn and the order alternating: the packed half-width
    NV12 depth stream against the existing u8 depth stream, with stm_stream_maps' format 1 (no maps) and with the default maps.
usage: python tools/depth_video_time.py [--stream-frames M] [--stream-runs R] [--kernel-trace FILE.csv] [--discard K] [--out FILE.json]
       [--profile-run [--in-flight N]]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = (-32.0, 32.0)  # lo, hi of the codes: the disparity range of D = 64, zero_disp = 32
KERNELS = ("stm_k_eye", "stm_k_front_pack")
PROFILE_FRAMES = 400


def quantise(d, maxcode):
    """stm_stream_maps' plane of a float map (include/stm_hip.h), in float32"""
    f = np.float32
    k = f(float(maxcode) / (float(f(LIMITS[1])) - float(f(LIMITS[0]))))
    t = (d.astype(f) - f(LIMITS[0])) * k
    t = np.minimum(np.maximum(t, f(0)), f(maxcode))
    return (t + f(0.5)).astype(np.uint8)


def squeeze_cols(a):
    """2 : 1 along the columns by pair averaging, as the drivers make a half-width frame"""
    a = a.astype(np.int32)
    return ((a[:, 0::2] + a[:, 1::2] + 1) >> 1).astype(np.uint8)


def to_nv12(bgr):
    """a BT.709 limited-range NV12 surface [H * 3 / 2][W] of a BGR picture (chroma: the mean of each 2 x 2 block)"""
    b, g, r = (bgr[..., i].astype(np.float64) for i in range(3))
    y = 16.0 + 0.1826 * r + 0.6142 * g + 0.0620 * b
    u = 128.0 - 0.1006 * r - 0.3386 * g + 0.4392 * b
    v = 128.0 + 0.4392 * r - 0.3989 * g - 0.0403 * b
    H, W = y.shape
    sub = lambda c: c.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))  # noqa: E731
    uv = np.empty((H // 2, W), np.float64)
    uv[:, 0::2], uv[:, 1::2] = sub(u), sub(v)
    return np.clip(np.rint(np.concatenate([y, uv], axis=0)), 0, 255).astype(np.uint8)


def run_frames(fs, frame, count, in_flight=2):
    pending = 0
    for _ in range(count):
        if pending == in_flight:
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


def kernel_trace_rows(path, discard):
    """per kernel name: the dispatches in time order, the first `discard` of every run of PROFILE_FRAMES dropped (each stream of the
    profile run launches its kernel once a frame)"""
    t = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if any(k in row["Kernel_Name"] for k in KERNELS):
                t.setdefault(row["Kernel_Name"], []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    out = {}
    for name, v in t.items():
        v = [d for _, d in sorted(v)]
        kept = [d for i, d in enumerate(v) if i % PROFILE_FRAMES >= discard]
        blocks = [v[i:i + PROFILE_FRAMES][discard:] for i in range(0, len(v), PROFILE_FRAMES)]  # one per stream that launched it
        out[name] = {"calls": len(v), "kept": len(kept), "median_us": float(np.median(kept)), "min_us": float(min(kept)),
                     "first_frames_median_us": float(np.median(v[:discard] or v)),
                     "per_stream": [{"median_us": float(np.median(b)), "min_us": float(min(b))} for b in blocks if b]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream-frames", type=int, default=3000)
    ap.add_argument("--stream-runs", type=int, default=3)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--discard", type=int, default=150)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--in-flight", type=int, default=1, choices=(1, 2), help="frames in flight during --profile-run")
    args = ap.parse_args()
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, synth, video
    stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    sbs = synth.tiled_sbs_frame(bud[0], bud[1], H, W)
    left, right = np.ascontiguousarray(sbs[:, :W]), np.ascontiguousarray(sbs[:, W:])
    fs = video.FrameStream(H, W, p)
    try:  # the pair's own left map: what the depth picture holds
        fs.submit(sbs)
        dl = np.array(fs.collect()[1])
    finally:
        fs.close()
    codes = quantise(dl, 255)
    grey = np.repeat(codes[:, :, None], 3, axis=2)
    fill = (1, 0.5)

    def depth_u8(**kw):
        return video.FrameStream(H, W, p, depth_input=("u8",) + LIMITS + fill, **kw)

    def packed(fmt, matrix, packing, filt, dfilter, **kw):
        return video.FrameStream(H, W, p, depth_video=(fmt, matrix, packing, 0, filt, 0, 0, dfilter, 4) + LIMITS + fill, **kw)
    fs = depth_u8()
    u8_frame = fs.pack_depth_frame(left, codes)
    fs.close()
    full_bgr = np.ascontiguousarray(np.concatenate([left, grey], axis=1))
    half_bgr = np.ascontiguousarray(np.concatenate([squeeze_cols(left), grey[:, 0::2]], axis=1))
    # (range 0: the grey of the depth half is the code itself; its Y after the conversion is not, which timing does not mind)
    video_streams = [("nv12_sbs_full", lambda **kw: packed("nv12", 1, 0, 0, 0, **kw), to_nv12(full_bgr)),
                     ("nv12_half_linear_dfilter1", lambda **kw: packed("nv12", 1, 1, 0, 1, **kw), to_nv12(half_bgr)),
                     ("nv12_half_catmull_rom_dfilter1", lambda **kw: packed("nv12", 1, 1, 1, 1, **kw), to_nv12(half_bgr)),
                     ("bgr_sbs_full", lambda **kw: packed("bgr", 0, 0, 0, 0, **kw), full_bgr)]
    if args.profile_run:
        half_pair = np.ascontiguousarray(np.concatenate([squeeze_cols(left), squeeze_cols(right)], axis=1))
        swapped = np.ascontiguousarray(np.concatenate([right, left], axis=1))  # (a full packing is `on` only with swap or a gap)
        stereo = [(dict(input_format="nv12", matrix=1, packing=(0, 1, 0, 0)), to_nv12(swapped)),
                  (dict(input_format="nv12", matrix=1, packing=(1, 0, 0, 0)), to_nv12(half_pair)),
                  (dict(input_format="nv12", matrix=1, packing=(1, 0, 1, 0)), to_nv12(half_pair)),
                  (dict(packing=(0, 1, 0, 0)), swapped)]
        # the stereo streams first: they load the chip, and the first light streams behind an idle chip run in a slow mode (DESIGN.md
        # sections 31 and 34).  Then the BGR form, the u8 depth stream, the NV12 forms, and the two half-width forms a second time
        packed_runs = [(make, frame) for _, make, frame in video_streams]
        runs = [((lambda kw=kw: video.FrameStream(H, W, p, **kw)), frame) for kw, frame in stereo]
        runs += [packed_runs[3], (depth_u8, u8_frame)] + packed_runs[:3] + packed_runs[1:3]
        for make, frame in runs:
            fs = make()
            try:
                run_frames(fs, frame, PROFILE_FRAMES, args.in_flight)
            finally:
                fs.close()
        print("profile run done")
        return
    out_bytes, maps = H * W * 3, 2 * H * W * 4
    half = video_streams[1]
    res = {"shape": [H, W], "content": "tiled bud pair: its left image and the pair's own left map as the depth picture", "limits": list(LIMITS),
           "fill": 1, "gate": 0.5, "dgate": 4, "stream_frames": args.stream_frames, "profile_frames_per_stream": PROFILE_FRAMES,
           "discarded_first_frames": args.discard,
           "bytes_per_frame": {"depth_u8": {"upload": int(u8_frame.nbytes), "download_default_maps": out_bytes + maps, "download_no_maps": out_bytes},
                               "packed_" + half[0]: {"upload": int(half[2].nbytes), "download_default_maps": out_bytes + maps,
                                                     "download_no_maps": out_bytes}}}
    if args.kernel_trace:
        res["kernel_trace_same_run"] = kernel_trace_rows(args.kernel_trace, args.discard)
    if args.stream_runs == 0:  # the kernel times alone
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    kinds = []
    for tag, kw in (("no_maps", dict(maps="none")), ("default_maps", {})):
        kinds.append(("packed_%s_%s" % (half[0], tag), (lambda kw=kw: half[1](**kw)), half[2]))
        kinds.append(("depth_u8_%s" % tag, (lambda kw=kw: depth_u8(**kw)), u8_frame))
    rates = {k: [] for k, _, _ in kinds}
    for i in range(args.stream_runs):
        for k, make, frame in (kinds if i % 2 == 0 else kinds[::-1]):
            rates[k].append(stream_rate(make, frame, args.stream_frames))
    res["stream_frames_per_s"] = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": v} for k, v in rates.items()}
    print(json.dumps(res["stream_frames_per_s"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
