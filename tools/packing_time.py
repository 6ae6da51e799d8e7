"""Cost and quality of packed input (stm_set_packing) at 1920 x 1080 per eye, D = 64, against the full side-by-side frame.

The full-resolution pair (the synthetic one bench.py times, and the tiled real-content bud pair) is packed by synth.pack_frame the way
a 3D encoder would (half packings: pairs averaged) and, for the NV12 forms, converted by synth.bgr_to_nv12 (matrix 0).  Forms: the
full side-by-side frame with packing off (the baseline: stm_k_front / stm_k_front_nv12), half-width side by side and half-height top
and bottom with either filter, full top and bottom, and (BGR only: the gap is odd) HDMI frame packing, top and bottom with 45 blank rows.
  - kernel time: stm_k_front_pack under stm_prof_* (its launcher carries the scope "front_pack"), one frame per form in turn, the
    order rotating, the median of --frames frames.  stm_k_front and stm_k_front_nv12 carry no event scope, and giving them one would
    touch the default path: they are read next to the twelve stm_k_front_pack instances from the rocprofv3 --kernel-trace --stats run
    of --profile-run, where all forms alternate, 20 frames each;
  - frame time, stages 3: HIP events around each frame call, the forms in turn, the order rotating, median and mean of --frames;
  - the frame stream's frames per second through its zero-copy entry points, two frames in flight, for full side-by-side NV12
    against half-width side-by-side NV12 (half the bytes again): the median, the least and the greatest of --stream-runs (3) fresh
    streams of --stream-frames frames each, the two alternating (--stream-only: nothing but this);
  - quality (evidence, not a gate), on the real-content pair: the mean absolute difference of the two maps and of the interlaced frame
    between the frame on the squeezed-and-expanded input (packings 1 and 3, both filters) and the frame on the unsqueezed pair.
usage: python tools/packing_time.py [--frames N] [--warmup W] [--stream-frames M] [--stream-runs R] [--stream-only] [--out FILE.json]
       [--profile-run]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (packing, swap, filter, gap); None = packing off on the full side-by-side frame
FORMS = [("full_sbs", None), ("half_sbs_linear", (1, 0, 0, 0)), ("half_sbs_catmull_rom", (1, 0, 1, 0)), ("full_tab", (2, 0, 0, 0)),
         ("half_tab_linear", (3, 0, 0, 0)), ("half_tab_catmull_rom", (3, 0, 1, 0)), ("frame_packing_gap45", (2, 0, 0, 45))]


def stream_rate(video, p, H, W, frame, packing, n):
    """frames per second of an NV12 FrameStream over n copies of `frame`, two in flight, zero-copy entry points"""
    fs = video.FrameStream(H, W, p, input_format="nv12", packing=packing)
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
    ap.add_argument("--stream-runs", type=int, default=3, help="fresh streams per form for the stream rate")
    ap.add_argument("--stream-only", action="store_true", help="only the stream rate")
    args = ap.parse_args()
    import torch
    import stm_amd
    from stm_amd import bmp_io, device_api as dev, synth, video
    stm_amd.lib()
    H, W, D, zd = 1080, 1920, 64, 32
    p = dev.FrameParams(num_disp=D, zero_disp=zd)
    bud = [bmp_io.read_bmp(os.path.join(ROOT, "tests", "golden", n)) for n in ("bud_2.bmp", "bud_3.bmp")]
    pairs = {"synthetic": synth.stereo_pair(H, W, D, zd)[:2], "real_content": synth.tiled_pair(bud[0], bud[1], H, W)}
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    res = {"shape": [H, W], "num_disp": D, "zero_disp": zd, "frames": args.frames, "warmup": args.warmup,
           "stream_frames": args.stream_frames, "matrix": 0, "forms": {n: pk for n, pk in FORMS}}
    for name, (L, R) in pairs.items():
        calls, host_nv12 = {}, {}
        for form, pk in FORMS:
            frame = synth.pack_frame(L, R, *((pk[0], pk[1], pk[3]) if pk else (0, 0, 0)))
            calls[("bgr", form)] = (pk, torch.from_numpy(frame).cuda())
            if frame.shape[0] % 2 == 0 and (pk is None or pk[3] % 2 == 0):
                y, uv = synth.bgr_to_nv12(frame, 0)
                calls[("nv12", form)] = (pk, torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())
                if form in ("full_sbs", "half_sbs_linear"):
                    host_nv12[form] = np.concatenate([y, uv], axis=0)
        keys = list(calls)

        def frame_call(key):
            c = calls[key]
            dev.set_packing(*(c[0] or (0, 0, 0, 0)))
            try:
                if key[0] == "bgr":
                    dev.d_adcensus_stm(c[1], dl, dr, out, p, stages=3)
                else:
                    dev.d_adcensus_stm_nv12(c[1], c[2], dl, dr, out, p, 3, 0)
            finally:
                dev.set_packing(0, 0, 0, 0)

        if args.profile_run:
            for _ in range(20):
                for key in keys:
                    frame_call(key)
            torch.cuda.synchronize()
            continue
        r = {}
        if not args.stream_only:
            # quality: every form's outputs against the full side-by-side frame of the same input format
            got = {}
            for key in keys:
                frame_call(key)
                torch.cuda.synchronize()
                got[key] = (dl.cpu().numpy().copy(), dr.cpu().numpy().copy(), out.cpu().numpy().astype(np.int32))
            quality = {}
            for key in keys:
                ref = got[(key[0], "full_sbs")]
                quality["%s_%s" % key] = {"mad_disp_l": float(np.abs(got[key][0] - ref[0]).mean()),
                                          "mad_disp_r": float(np.abs(got[key][1] - ref[1]).mean()),
                                          "mad_interlaced": float(np.abs(got[key][2] - ref[2]).mean())}
            r["quality_vs_full_sbs"] = quality
            del got
            for _ in range(args.warmup):
                for key in keys:
                    frame_call(key)
            torch.cuda.synchronize()
            ms = {key: [] for key in keys}
            for i in range(args.frames):
                for key in keys[i % len(keys):] + keys[:i % len(keys)]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    frame_call(key)
                    e1.record()
                    e1.synchronize()
                    ms[key].append(e0.elapsed_time(e1))
            r["frame_ms"] = {"%s_%s" % key: {"median": float(np.median(ms[key])), "mean": float(np.mean(ms[key]))} for key in keys}
            # stm_k_front_pack under the library's own event scopes
            packed = [key for key in keys if calls[key][0] is not None]
            us = {key: [] for key in packed}
            dev.prof_enable(True)
            try:
                for i in range(args.frames):
                    for key in packed[i % len(packed):] + packed[:i % len(packed)]:
                        dev.prof_reset()
                        frame_call(key)
                        torch.cuda.synchronize()
                        n, t = dev.prof_read("front_pack")
                        assert n == 1
                        us[key].append(t * 1e3)
            finally:
                dev.prof_enable(False)
                dev.prof_reset()
            r["front_pack_us_median"] = {"%s_%s" % key: float(np.median(us[key])) for key in packed}
        calls.clear()
        rates = {form: [] for form in host_nv12}
        forms = list(host_nv12)
        for i in range(args.stream_runs):  # a fresh stream per run, the two forms alternating
            for form in (forms if i % 2 == 0 else forms[::-1]):
                rates[form].append(stream_rate(video, p, H, W, host_nv12[form], dict(FORMS)[form], args.stream_frames))
        r["stream_nv12_frames_per_s"] = {form: {"median": float(np.median(rates[form])), "min": float(min(rates[form])),
                                                "max": float(max(rates[form])), "runs": rates[form],
                                                "input_bytes_per_frame": int(host_nv12[form].size)} for form in forms}
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
