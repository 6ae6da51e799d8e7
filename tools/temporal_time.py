"""Cost of the temporal disparity stabilisation (stages bit 0x2000) at 1920 x 1080, D = 64, default parameters.

For the synthetic frame bench.py times and the tiled real-content bud pair, each as a pair of consecutive frames (the frame and
the same frame under independent noise in {-2 .. 2} per channel, the static noisy scene the step is made for):
  - frame time of stm_d_adcensus_stm_t with stages 3 against 3 | 0x2000 (history: the previous frame and its maps), the two
    alternating frame by frame in one process, HIP events around each frame (after a warm-up), median and mean;
  - the `temporal` kernel (one launch, both views) from stm_prof_read, one profiled frame at a time (the kernel it is compared
    with, stm_k_front, carries no event scope: its time is in the rocprofv3 statistics of --profile-run);
  - how many map elements the step changes, and the share of pixels each gate refuses;
  - the frame stream's frames per second with and without the bit, through its zero-copy entry points, two frames in flight:
    with the bit the two frames no longer overlap on the GPU.
usage: python tools/temporal_time.py [--frames N] [--warmup W] [--stream-frames M] [--out FILE.json] [--profile-run]
--profile-run: only a few frames of each kind (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEMPORAL = 0x2000


def noisy(frame, seed):
    rng = np.random.RandomState(seed)
    return np.clip(frame.astype(np.int16) + rng.randint(-2, 3, size=frame.shape).astype(np.int16), 0, 255).astype(np.uint8)


def stream_rate(video, p, H, W, pair, stages, n):
    """frames per second of a FrameStream over n frames alternating between the two frames of `pair`, two in flight, frames
    written into the pinned input buffer and results read as views (no host copies besides the one into the pinned buffer)"""
    fs = video.FrameStream(H, W, p, stages=stages)
    try:
        def run(count):
            pending = 0
            for k in range(count):
                if pending == 2:
                    fs.collect_view()
                    pending -= 1
                fs.input_buffer()[...] = pair[k & 1]
                assert fs.submit_inplace() >= 0
                pending += 1
            while pending:
                fs.collect_view()
                pending -= 1
        run(8)  # eager and captured frames of both slots
        t0 = time.perf_counter()
        run(n)
        return n / (time.perf_counter() - t0)
    finally:
        fs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--stream-frames", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true")
    args = ap.parse_args()
    import torch
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, synth, video
    stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    frames = {"synthetic": synth.sbs_frame(H, W, D, zd)[0], "real_content": synth.tiled_sbs_frame(bud[0], bud[1], H, W)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    ql, qr = torch.zeros_like(dl), torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    both = (3, 3 | TEMPORAL)

    def frame(d_sbs, d_prev, st):
        dev.d_adcensus_stm_t(d_sbs, dl, dr, out, p, st, d_prev, ql, qr)

    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "frames": args.frames, "warmup": args.warmup,
           "stream_frames": args.stream_frames, "parameters": list(dev.TEMPORAL_DEFAULTS)}
    for name, sbs in frames.items():
        pair = [noisy(sbs, 1), noisy(sbs, 2)]
        d_prev, d_sbs = torch.from_numpy(pair[0]).cuda(), torch.from_numpy(pair[1]).cuda()
        # the history maps: what the previous frame puts out
        dev.d_adcensus_stm(d_prev, ql, qr, out, p, stages=3)
        torch.cuda.synchronize()
        if args.profile_run:
            for st in both * 5:
                frame(d_sbs, d_prev, st)
            torch.cuda.synchronize()
            continue
        for _ in range(args.warmup):
            for st in both:
                frame(d_sbs, d_prev, st)
        torch.cuda.synchronize()
        ms = {st: [] for st in both}
        for i in range(args.frames):
            for st in (both if i % 2 == 0 else both[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                frame(d_sbs, d_prev, st)
                e1.record()
                e1.synchronize()
                ms[st].append(e0.elapsed_time(e1))
        r = {}
        for st, key in zip(both, ("stages3", "stages3_temporal")):
            a = np.array(ms[st])
            r[key + "_ms_median"] = float(np.median(a))
            r[key + "_ms_mean"] = float(a.mean())
        r["frame_delta_ms_median"] = r["stages3_temporal_ms_median"] - r["stages3_ms_median"]
        r["frame_delta_share"] = r["frame_delta_ms_median"] / r["stages3_ms_median"]
        nprof, t_k = 20, 0.0
        dev.prof_enable(True)
        for i in range(nprof):
            dev.prof_reset()
            frame(d_sbs, d_prev, 3 | TEMPORAL)
            torch.cuda.synchronize()
            n_t, tt = dev.prof_read("temporal")
            assert n_t == 1, n_t
            t_k += tt
        dev.prof_enable(False)
        dev.prof_reset()
        r["temporal_kernel_ms"] = t_k / nprof
        # algorithmic traffic: two images of 3 bytes, two maps read, one written (the latter only where the gates pass)
        r["temporal_kernel_algorithmic_bytes"] = 2 * H * W * (2 * 3 + 3 * 4)
        r["temporal_kernel_gbytes_per_s"] = r["temporal_kernel_algorithmic_bytes"] / (r["temporal_kernel_ms"] * 1e-3) / 1e9
        maps = {}
        for st in both:
            frame(d_sbs, d_prev, st)
            torch.cuda.synchronize()
            maps[st] = (dl.cpu().numpy().copy(), dr.cpu().numpy().copy())
        prev_l = ql.cpu().numpy()
        diff = np.abs(maps[3][0] - maps[3 | TEMPORAL][0])
        r["left_map_share_changed"] = float(np.mean(diff != 0))
        r["left_map_share_refused_by_disparity_gate"] = float(np.mean(np.abs(prev_l - maps[3][0]) > dev.TEMPORAL_DEFAULTS[2]))
        r["left_map_mean_abs_change_vs_previous_frame_without"] = float(np.mean(np.abs(maps[3][0] - prev_l)))
        r["left_map_mean_abs_change_vs_previous_frame_with"] = float(np.mean(np.abs(maps[3 | TEMPORAL][0] - prev_l)))
        del d_prev, d_sbs
        rates = {st: [] for st in both}
        for i in range(3):  # a fresh stream per run, the two forms alternating
            for st in (both if i % 2 == 0 else both[::-1]):
                rates[st].append(stream_rate(video, p, H, W, pair, st, args.stream_frames))
        for st, key in zip(both, ("stream_frames_per_s", "stream_frames_per_s_temporal")):
            r[key] = float(np.median(rates[st]))
            r[key + "_runs"] = rates[st]
        r["stream_rate_ratio"] = r["stream_frames_per_s_temporal"] / r["stream_frames_per_s"]
        res[name] = r
        print(name, json.dumps(r), flush=True)
    if args.profile_run:
        print("profile run done")
        return
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
