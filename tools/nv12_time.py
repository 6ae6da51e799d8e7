"""Cost of NV12 input at 1920 x 1080, D = 64, against the BGR calls on the same content.

For the synthetic frame bench.py times and the tiled real-content bud pair, each converted to NV12 by synth.bgr_to_nv12 (matrix 0)
and, for the BGR calls, back to BGR by the library's own stm_d_demux_nv12, so both forms compute the same frame:
  - frame time, stages 3: stm_d_adcensus_stm on the BGR frame against stm_d_adcensus_stm_nv12 on the two planes, alternating frame
    by frame in one process, HIP events around each frame (after a warm-up), median and mean; the outputs are compared once;
  - the frame stream's frames per second with BGR and with NV12 input through its zero-copy entry points, two frames in flight:
    the median of three streams of --stream-frames frames each, the two formats alternating.  The stream exposes no per-direction
    copy times, so none are reported.
stm_k_front carries no event scope, and giving it one would touch the default path: the two front kernels are compared in the
rocprofv3 --kernel-trace --stats run of --profile-run, where the two frame calls alternate, 20 frames each per content.
usage: python tools/nv12_time.py [--frames N] [--warmup W] [--stream-frames M] [--out FILE.json] [--profile-run]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stream_rate(video, p, H, W, frame, fmt, n):
    """frames per second of a FrameStream over n copies of `frame`, two in flight, written into the pinned input buffer and read
    as views (no host copies besides the one into the pinned buffer)"""
    fs = video.FrameStream(H, W, p, input_format=fmt)
    try:
        def run(count):
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
    ap.add_argument("--stream-frames", type=int, default=1000)
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
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    forms = ("bgr", "nv12")
    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "frames": args.frames, "warmup": args.warmup,
           "stream_frames": args.stream_frames, "matrix": 0,
           "input_bytes_per_frame": {"bgr": H * 2 * W * 3, "nv12": H * 2 * W * 3 // 2}}
    for name, sbs in frames.items():
        y, uv = synth.bgr_to_nv12(sbs, 0)
        d_y, d_uv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
        il = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
        ir = torch.zeros_like(il)
        dev.d_demux_nv12(il, ir, d_y, d_uv, 0)
        d_sbs = torch.cat([il, ir], dim=1).contiguous()  # the BGR frame of the same content
        del il, ir

        def frame(form):
            if form == "bgr":
                dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=3)
            else:
                dev.d_adcensus_stm_nv12(d_y, d_uv, dl, dr, out, p, 3, 0)

        if args.profile_run:
            for form in forms * 20:
                frame(form)
            torch.cuda.synchronize()
            continue
        got = {}
        for form in forms:
            frame(form)
            torch.cuda.synchronize()
            got[form] = (dl.cpu().numpy().copy(), dr.cpu().numpy().copy(), out.cpu().numpy().copy())
        r = {"outputs_equal": all(np.array_equal(a, b) for a, b in zip(got["bgr"], got["nv12"]))}
        del got
        for _ in range(args.warmup):
            for form in forms:
                frame(form)
        torch.cuda.synchronize()
        ms = {form: [] for form in forms}
        for i in range(args.frames):
            for form in (forms if i % 2 == 0 else forms[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                frame(form)
                e1.record()
                e1.synchronize()
                ms[form].append(e0.elapsed_time(e1))
        for form in forms:
            a = np.array(ms[form])
            r["frame_%s_ms_median" % form] = float(np.median(a))
            r["frame_%s_ms_mean" % form] = float(a.mean())
        r["frame_delta_ms_median"] = r["frame_nv12_ms_median"] - r["frame_bgr_ms_median"]
        r["frame_ratio"] = r["frame_nv12_ms_median"] / r["frame_bgr_ms_median"]
        host = {"bgr": d_sbs.cpu().numpy(), "nv12": np.concatenate([y, uv], axis=0)}
        del d_sbs, d_y, d_uv
        rates = {form: [] for form in forms}
        for i in range(3):  # a fresh stream per run, the two formats alternating
            for form in (forms if i % 2 == 0 else forms[::-1]):
                rates[form].append(stream_rate(video, p, H, W, host[form], form, args.stream_frames))
        for form in forms:
            r["stream_%s_frames_per_s" % form] = float(np.median(rates[form]))
            r["stream_%s_frames_per_s_runs" % form] = rates[form]
        r["stream_rate_ratio"] = r["stream_nv12_frames_per_s"] / r["stream_bgr_frames_per_s"]
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
