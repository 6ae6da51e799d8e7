"""The reduced-resolution frame for frame sequences on the GPU: stm_d_adcensus_stm_2t and stm_d_adcensus_stm_2nv12 bit for bit
against test_reduced_stream_ref.reduced_frame_ref, the fused front against the chain (stm_set_agg_variant(600)), the default path
against the oracle, a FrameStream with match= against the per-frame calls (eager, capture and replay in both slots), the setters'
rules, and the real-content bud pair through a stream."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_nv12_ref import nv12_frame, nv12_to_bgr_ref
from test_reduced_stream_ref import TEMPORAL, frame_case, reduced_frame_ref
from test_temporal_ref import SEQ, mixed_sequence
from test_upsample_ref import GUIDED_UP, INTERP, LINEAR_WARP, SUBPIXEL

pytestmark = pytest.mark.gpu

WORDS = [3, 3 | GUIDED_UP | LINEAR_WARP, 3 | INTERP | SUBPIXEL, 3 | TEMPORAL, 3 | TEMPORAL | GUIDED_UP]
WORD_IDS = ["0x%x" % s for s in WORDS]


def _params(p):
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=p.num_disp, zero_disp=p.zero_disp, usd=p.usd, lsd=p.lsd)


def _second(sbs):
    """the next frame of a sequence: the same scene under a little noise, so pixels fall on both sides of the colour gate"""
    rng = np.random.RandomState(5)
    return np.clip(sbs.astype(np.int32) + rng.randint(-3, 4, size=sbs.shape), 0, 255).astype(np.uint8)


def call_2t(sbs, p, h, w, scale, stages, hist=None, out_shape=None):
    """stm_d_adcensus_stm_2t; hist = (previous frame, previous disp_l, previous disp_r) or None.  Returns (disp_l, disp_r, interlaced)."""
    import torch
    from stm_amd import device_api as dev
    H, W = sbs.shape[0], sbs.shape[1] // 2
    Ho, Wo = out_shape or (H, W)
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(Ho, Wo, 3, dtype=torch.uint8, device="cuda")
    hs = [None] * 3 if hist is None else [torch.from_numpy(np.array(a)).cuda() for a in hist]
    dev.d_adcensus_stm_2t(torch.from_numpy(np.array(sbs)).cuda(), dl, dr, out, p, h, w, scale, stages, *hs)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def call_2nv12(y, uv, p, h, w, scale, stages, hist=None, matrix=0, out_shape=None):
    """stm_d_adcensus_stm_2nv12; hist = (previous img_l, img_r, disp_l, disp_r) or None.  Returns (disp_l, disp_r, interlaced, img_l, img_r)."""
    import torch
    from stm_amd import device_api as dev
    H, W = y.shape[0], y.shape[1] // 2
    Ho, Wo = out_shape or (H, W)
    dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    dr = torch.zeros_like(dl)
    out = torch.zeros(Ho, Wo, 3, dtype=torch.uint8, device="cuda")
    il, ir = (torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda") for _ in range(2))
    hs = [None] * 4 if hist is None else [torch.from_numpy(np.array(a)).cuda() for a in hist]
    dev.d_adcensus_stm_2nv12(torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(np.array(uv)).cuda(), dl, dr, out, p, h, w, scale, stages,
                             matrix, il, ir, *hs)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy(), il.cpu().numpy(), ir.cpu().numpy()


def _equal(got, want, what):
    for j in range(3):
        assert np.array_equal(got[j], want[j]), (what, j)


# ----------------------------------------------------------------------------- 1. the device calls against the reference
@pytest.mark.parametrize("stages", WORDS, ids=WORD_IDS)
@pytest.mark.parametrize("k", [0, 1], ids=["48x100", "37x83"])
def test_2t_against_the_reference(gpu_ready, orc, k, stages):
    """the first frame (no history: the temporal bit does nothing), and with the bit a second frame against the first one's"""
    sbs, p0, h, w, scale = frame_case(k)
    p = _params(p0)
    want = reduced_frame_ref(orc, sbs, p0, h, w, scale, stages & ~3)
    got = call_2t(sbs, p, h, w, scale, stages)
    _equal(got, want, "first frame")
    if stages & TEMPORAL:
        nxt = _second(sbs)
        want2 = reduced_frame_ref(orc, nxt, p0, h, w, scale, stages & ~3, hist=(sbs, want[0], want[1]))
        assert not np.array_equal(want2[0], reduced_frame_ref(orc, nxt, p0, h, w, scale, stages & ~3 & ~TEMPORAL)[0])  # the step acts
        _equal(call_2t(nxt, p, h, w, scale, stages, hist=(sbs, got[0], got[1])), want2, "second frame")


def _nv12_case(k):
    """frame_case(k) as NV12 planes: cropped to even sizes (NV12's rule; 37 x 83 becomes 36 x 82, still matched at 19 x 41), with the
    BGR frame the conversion defines"""
    from stm_amd import synth
    sbs, p0, h, w, scale = frame_case(k)
    H, W = sbs.shape[0] & ~1, (sbs.shape[1] // 2) & ~1
    W0 = sbs.shape[1] // 2
    even = np.ascontiguousarray(np.concatenate([sbs[:H, :W], sbs[:H, W0:W0 + W]], axis=1))
    y, uv = synth.bgr_to_nv12(even)
    return y, uv, nv12_to_bgr_ref(y, uv), p0, h, w, scale


@pytest.mark.parametrize("stages", WORDS, ids=WORD_IDS)
@pytest.mark.parametrize("k", [0, 1], ids=["48x100", "36x82"])
def test_2nv12_against_the_reference(gpu_ready, orc, k, stages):
    from stm_amd import synth
    y, uv, bgr, p0, h, w, scale = _nv12_case(k)
    p = _params(p0)
    W = bgr.shape[1] // 2
    want = reduced_frame_ref(orc, bgr, p0, h, w, scale, stages & ~3)
    got = call_2nv12(y, uv, p, h, w, scale, stages)
    _equal(got, want, "first frame")
    assert np.array_equal(got[3], bgr[:, :W]) and np.array_equal(got[4], bgr[:, W:])
    if stages & TEMPORAL:
        y2, uv2 = synth.bgr_to_nv12(_second(bgr))
        bgr2 = nv12_to_bgr_ref(y2, uv2)
        want2 = reduced_frame_ref(orc, bgr2, p0, h, w, scale, stages & ~3, hist=(bgr, want[0], want[1]))
        _equal(call_2nv12(y2, uv2, p, h, w, scale, stages, hist=(got[3], got[4], got[0], got[1])), want2, "second frame")


# ----------------------------------------------------------------------------- 2. fused against unfused, and the default path
def test_variant_600_gives_the_same_arrays(gpu_ready, stm):
    lib = stm.lib()
    sbs, p0, h, w, scale = frame_case(1)
    p = _params(p0)
    y, uv, _, _, _, _, _ = _nv12_case(0)
    h0, w0, s0 = frame_case(0)[2:]
    nxt = _second(sbs)

    def run():
        a = call_2t(sbs, p, h, w, scale, 3 | TEMPORAL | GUIDED_UP | LINEAR_WARP)
        b = call_2t(nxt, p, h, w, scale, 3 | TEMPORAL | GUIDED_UP | LINEAR_WARP, hist=(sbs, a[0], a[1]))
        c = call_2nv12(y, uv, p, h0, w0, s0, 3 | INTERP)
        d = call_2t(sbs, p, h, w, scale, 3, out_shape=(50, 121))
        return a + b + c + d
    fused = run()
    lib.stm_set_agg_variant(600)
    try:
        chain = run()
    finally:
        lib.stm_set_agg_variant(0)
    assert len(fused) == len(chain) and all(np.array_equal(a, b) for a, b in zip(fused, chain))


def test_default_path_is_the_oracle_before_and_after(gpu_ready, orc):
    import torch
    from stm_amd import device_api as dev
    sbs, p0, h, w, scale = frame_case(0)
    p = _params(p0)
    H, W = sbs.shape[0], sbs.shape[1] // 2
    o = orc.adcensus_stm_2(sbs, H, W, h, w, scale, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd,
                           p.usd, p.lsd, p.thresh_s, p.thresh_h)

    def default():
        dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
        dr = torch.zeros_like(dl)
        out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
        dev.d_adcensus_stm_2s(torch.from_numpy(sbs).cuda(), dl, dr, out, p, h, w, scale, stages=3)
        torch.cuda.synchronize()
        _equal((dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()), (o["disp_l"], o["disp_r"], o["interlaced"]), "2s")
    default()
    first = call_2t(sbs, p, h, w, scale, 3 | TEMPORAL | GUIDED_UP)
    call_2t(_second(sbs), p, h, w, scale, 3 | TEMPORAL | GUIDED_UP, hist=(sbs, first[0], first[1]))
    default()


# ----------------------------------------------------------------------------- 3. a stream with match=
MATCH = (SEQ["H"] // 2, SEQ["W"] // 2, 0.5)
QUILT, DEPTH = (1, 4, 2, 3, 1), (1.5, 0.75)


def _seq_params():
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=SEQ["D"], zero_disp=SEQ["zd"], usd=SEQ["usd"], lsd=SEQ["lsd"])


def _run_stream(frames, p, stages, input_format="bgr", H=SEQ["H"], W=SEQ["W"], match=MATCH, **kw):
    from stm_amd import video
    fs = video.FrameStream(H, W, p, stages=stages, input_format=input_format, match=match, **kw)
    try:
        got, pending = [], 0
        for f in frames:
            if pending == 2:
                got.append(fs.collect())
                pending -= 1
            assert fs.submit(f) >= 0
            pending += 1
        while pending:
            got.append(fs.collect())
            pending -= 1
    finally:
        fs.close()
    assert [g[0] for g in got] == list(range(len(frames)))
    return got


def stream_check(stages, nv12=False, scoped=False, n=6):
    """n frames through a stream with a match size (both slots run eager, capture and replay): every collected frame equals the
    device call on the same input and the previous collected frame as its history.  scoped: the stream carries a quilt layout and
    a manual depth budget, and the device call runs under the same two settings of the thread."""
    from stm_amd import device_api as dev, synth
    p = _seq_params()
    frames = mixed_sequence(n)
    h, w, scale = MATCH
    kw = dict(layout=QUILT, depth=DEPTH) if scoped else {}
    if nv12:
        planes = [synth.bgr_to_nv12(f) for f in frames]
        got = _run_stream([nv12_frame(y, uv) for y, uv in planes], p, stages, "nv12", **kw)
    else:
        got = _run_stream(frames, p, stages, **kw)
    if scoped:
        dev.set_layout(*QUILT)
        dev.set_depth(1, *DEPTH)
    try:
        prev = None
        for k in range(n):
            temporal = bool(stages & TEMPORAL) and k > 0
            if nv12:
                want = call_2nv12(*planes[k], p, h, w, scale, stages, hist=(prev[3], prev[4], prev[0], prev[1]) if temporal else None)
            else:
                want = call_2t(frames[k], p, h, w, scale, stages, hist=(frames[k - 1], prev[0], prev[1]) if temporal else None)
            _equal(got[k][1:], want, "frame %d" % k)
            prev = want
    finally:
        if scoped:
            dev.set_layout(0)
            dev.set_depth(0)


@pytest.mark.parametrize("nv12", [False, True], ids=["bgr", "nv12"])
@pytest.mark.parametrize("stages", [3, 3 | GUIDED_UP | LINEAR_WARP, 3 | TEMPORAL | GUIDED_UP], ids=["0x3", "0x1803", "0x3003"])
def test_stream_with_match_size(gpu_ready, stages, nv12):
    stream_check(stages, nv12)


def test_stream_scopes_reach_the_reduced_frame(gpu_ready):
    """a quilt layout and a manual depth budget of the stream: the frames differ from the unscoped stream's and equal the scoped call's"""
    stream_check(3 | TEMPORAL, scoped=True)
    plain = _run_stream(mixed_sequence(2), _seq_params(), 3)
    scoped = _run_stream(mixed_sequence(2), _seq_params(), 3, layout=QUILT, depth=DEPTH)
    assert np.array_equal(plain[1][1], scoped[1][1]) and not np.array_equal(plain[1][3], scoped[1][3])


def test_stream_without_graphs_in_a_child_process(gpu_ready):
    """STM_STREAM_GRAPH is read when the stream is created: a fresh child process"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_reduced_stream as t\n"
            "t.stream_check(3 | t.TEMPORAL | t.GUIDED_UP)\n"
            "t.stream_check(3, nv12=True)\n"
            "print('ok')\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, STM_STREAM_GRAPH="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ----------------------------------------------------------------------------- 4. the setters' rules
def test_setter_rules(gpu_ready, stm):
    from stm_amd import video
    lib = stm.lib()
    p = _seq_params()
    H, W = SEQ["H"], SEQ["W"]
    lib.stm_set_error_mode(1)
    fs, fs2 = video.FrameStream(H, W, p), video.FrameStream(H, W, p)
    try:
        def refused(call, *words):
            lib.stm_d_filter_median(None, 0, 0)  # plant a known message
            assert call() == -1
            err = lib.stm_last_error()
            assert all(wd in err for wd in words), err
        sm, ss, sp = lib.stm_stream_set_match_size, lib.stm_stream_set_stages, lib.stm_stream_set_packing
        # without a match size 0x1000 stays refused with the message the full-resolution stream always gave
        refused(lambda: ss(fs._h, 3 | 0x1000), b"stream_set_stages", b"0x1000", b"reduced-resolution frame")
        for bad in ((0, 5, 0.5), (5, 0, 0.5), (-1, -1, 0.5), (4, -2, 0.5)):
            refused(lambda: sm(fs._h, *bad), b"stream_set_match_size", b"num_rows_disp")
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            refused(lambda: sm(fs._h, 20, 36, bad), b"stream_set_match_size", b"disp_scale")
        assert sm(fs._h, 0, 0, float("nan")) == 0  # off: the scale is not looked at
        assert sm(fs._h, 20, 36, 0.5) == 0
        for bad in (3 | 0x100, 3 | 0x4000, 3 | 0x1000 | 0x100, 2 | 0x1000, 3 | 0x8000):
            refused(lambda: ss(fs._h, bad), b"stream_set_stages")
        assert ss(fs._h, 3 | 0x1000 | 0x2000 | 0x800 | 0x400 | 0x200) == 0
        refused(lambda: sm(fs._h, 0, 0, 1.0), b"stream_set_match_size", b"0x1000")  # off while the stages hold 0x1000
        assert ss(fs._h, 3) == 0 and sm(fs._h, 0, 0, 1.0) == 0
        refused(lambda: ss(fs._h, 3 | 0x1000), b"stream_set_stages", b"0x1000")
        # a packing and a match size, in either order
        assert sm(fs._h, 20, 36, 0.5) == 0
        refused(lambda: sp(fs._h, 0, 1, 0, 0), b"stream_set_packing", b"match size")
        assert sp(fs._h, 0, 0, 0, 0) == 0
        assert sp(fs2._h, 0, 1, 0, 0) == 0
        refused(lambda: sm(fs2._h, 20, 36, 0.5), b"stream_set_match_size", b"packing")
        assert sp(fs2._h, 0, 0, 0, 0) == 0 and sm(fs2._h, 20, 36, 0.5) == 0
        # after the first submit every setter is closed
        assert ss(fs._h, 3 | 0x1000) == 0
        assert fs.submit(mixed_sequence(1)[0]) == 0
        refused(lambda: sm(fs._h, 10, 18, 0.25), b"stream_set_match_size", b"first submit")
        refused(lambda: sm(fs._h, 0, 0, 1.0), b"stream_set_match_size", b"first submit")
        refused(lambda: ss(fs._h, 3), b"stream_set_stages", b"first submit")
        refused(lambda: sp(fs._h, 0, 0, 0, 0), b"stream_set_packing", b"first submit")
        assert fs.collect()[0] == 0
        with pytest.raises(ValueError, match="stm_stream_set_match_size"):
            video.FrameStream(H, W, p, match=(0, 3, 0.5))
    finally:
        lib.stm_set_error_mode(0)
        fs.close()
        fs2.close()


# ----------------------------------------------------------------------------- 5. full size
def test_bud_pair_through_a_stream(gpu_ready):
    """The real-content bud pair (640 x 384) matched at 320 x 192, D = 16: three frames through a stream with 0x1000 and 0x2000,
    against the per-frame calls"""
    from stm_amd import bmp_io, device_api as dev
    L, R = bmp_io.read_bmp(os.path.join(GOLDEN, "bud_2.bmp")), bmp_io.read_bmp(os.path.join(GOLDEN, "bud_3.bmp"))
    sbs = np.ascontiguousarray(np.concatenate([L, R], axis=1))
    H, W = L.shape[:2]
    assert (H, W) == (384, 640)
    p = dev.FrameParams(num_disp=16, zero_disp=8)
    stages = 3 | GUIDED_UP | TEMPORAL
    frames = [sbs, _second(sbs), sbs]
    got = _run_stream(frames, p, stages, H=H, W=W, match=(192, 320, 0.5))
    prev = None
    for k, f in enumerate(frames):
        want = call_2t(f, p, 192, 320, 0.5, stages, hist=(frames[k - 1], prev[0], prev[1]) if k else None)
        _equal(got[k][1:], want, "frame %d" % k)
        prev = want
    assert np.unique(got[2][1]).size > 8  # a real map, not a constant
