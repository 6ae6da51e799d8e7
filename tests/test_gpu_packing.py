"""Packed stereo frames on the GPU: the unpacking as a stage (stm_demux_packed / stm_demux_nv12_packed, both flavours), the
device-resident frame under stm_set_packing and the frame stream under stm_stream_set_packing, every comparison bit for bit: the
stage against the numpy statement of the definition (test_packing_ref.unpack_ref / unpack_nv12_ref), the frame and the stream
against the same calls, packing off, on the unpacked side-by-side frame that statement builds."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_nv12_ref import nv12_frame, random_planes
from test_packing_ref import SETTINGS, build_frame, frame_shape, random_eyes, unpack_nv12_ref, unpack_ref, unpacked_sbs
from test_temporal_ref import ALPHA, THRESH_COLOR, THRESH_DISP, sad_max, temporal_ref

pytestmark = pytest.mark.gpu

T, SUBPIXEL, INTERP, LINEAR_WARP = 0x2000, 0x200, 0x400, 0x800
assert (ALPHA, THRESH_COLOR, THRESH_DISP) == (0.5, 24, 1.5)  # a frame sequence's defaults (stm_hip.h)
FILL = 0x5A
SETTING_IDS = ["p%d_s%d_f%d" % s for s in SETTINGS]
H, W, D, ZD = 36, 132, 16, 8  # the frame tests' eye: three tile columns (the last partial), three tile rows (the last partial)


def _params():
    from stm_amd import device_api as dev
    return dev.FrameParams(num_disp=D, zero_disp=ZD, usd=17, lsd=8)


def _gap(setting):
    """0 and 6 both occur for every packing"""
    return 6 if (setting[1] + setting[2]) % 2 == 0 else 0


# ----------------------------------------------------------------------------- 1. the stage
@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
def test_demux_packed_both_flavours(gpu_ready, stm, setting):
    """(22, 70) and (36, 132) straddle the 256-thread rows of the stage kernel; gap 0 and 6, 3- and 4-byte pixels, a row three pixels
    longer than the rule asks, the gap and the spare columns full of noise, every device buffer at an odd address in one arena"""
    import torch
    from test_gpu_caller_buffers import Arena, P, read
    from stm_amd import host_api as api
    lib = stm.lib()
    lib.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for (h, w), gap, E in [((22, 70), 0, 3), ((22, 70), 6, 4), ((36, 132), 6, 3), ((36, 132), 0, 4)]:
        frame3 = build_frame(random_eyes(h + w + gap, h, w, setting[0]), h, w, setting, gap, extra_cols=3, seed=E)
        frame = np.full(frame3.shape[:2] + (E,), 0xC3, np.uint8)
        frame[:, :, :3] = frame3
        want = unpack_ref(frame3, h, w, setting, gap)
        pk = (setting[0], setting[1], setting[2], gap)
        got = api.demux_packed(frame, h, w, pk)
        for g, wv in zip(got, want):
            assert np.array_equal(g[:, :, :3], wv) and (g[:, :, 3:] == 0).all(), ("host", h, w, gap, E)
        arena = Arena(True, nbytes=1 << 20)
        d_f = arena.put(frame, 1)
        d_l, d_r = arena.put(np.full((h, w, E), FILL, np.uint8), 5), arena.put(np.full((h, w, E), FILL, np.uint8), 7)
        lib.stm_d_demux_packed(P(d_l), P(d_r), P(d_f), h, frame.shape[1], w, E, *pk)
        assert arena.intact(), (h, w, gap, E)
        for d, wv in ((d_l, want[0]), (d_r, want[1])):
            g = read(d, np.uint8, (h, w, E))
            assert np.array_equal(g[:, :, :3], wv), ("device", h, w, gap, E)
            assert (g[:, :, 3:] == FILL).all()  # left to the caller
        assert np.array_equal(read(d_f, np.uint8, frame.shape), frame)


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
def test_demux_nv12_packed_both_flavours(gpu_ready, stm, setting):
    """(20, 68) and (36, 132); gap 0 and 6; both pitches above the minimum and different; planes and images at odd addresses"""
    import torch
    from test_gpu_caller_buffers import Arena, P, read
    from stm_amd import host_api as api
    lib = stm.lib()
    lib.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for (h, w), gap, E, matrix in [((20, 68), 0, 3, 0), ((20, 68), 6, 4, 1), ((36, 132), 6, 3, 2), ((36, 132), 0, 4, 3)]:
        rows_f, need = frame_shape(h, w, setting[0], gap)
        Wsbs, pitch_y, pitch_uv = need + 2, need + 10, need + 6
        y, uv = random_planes(h * 7 + w + gap, rows_f, Wsbs, pitch_y, pitch_uv)
        want = unpack_nv12_ref(y, uv, h, w, setting, gap, matrix)
        pk = (setting[0], setting[1], setting[2], gap)
        got = api.demux_nv12_packed(y, uv, h, w, pk, E, matrix, num_cols_sbs=Wsbs)
        for g, wv in zip(got, want):
            assert np.array_equal(g[:, :, :3], wv) and (g[:, :, 3:] == 0).all(), ("host", h, w, gap, E)
        ybuf = np.full(rows_f * pitch_y, 0xC3, np.uint8)
        uvbuf = np.full((rows_f // 2) * pitch_uv, 0xC3, np.uint8)
        ybuf.reshape(rows_f, pitch_y)[:, :Wsbs] = y
        uvbuf.reshape(rows_f // 2, pitch_uv)[:, :uv.shape[1]] = uv
        arena = Arena(True, nbytes=1 << 20)
        d_y, d_uv = arena.put(ybuf, 1), arena.put(uvbuf, 3)
        d_l, d_r = arena.put(np.full((h, w, E), FILL, np.uint8), 5), arena.put(np.full((h, w, E), FILL, np.uint8), 7)
        lib.stm_d_demux_nv12_packed(P(d_l), P(d_r), P(d_y), pitch_y, P(d_uv), pitch_uv, h, Wsbs, w, E, matrix, *pk)
        assert arena.intact(), (h, w, gap, E)
        for d, wv in ((d_l, want[0]), (d_r, want[1])):
            g = read(d, np.uint8, (h, w, E))
            assert np.array_equal(g[:, :, :3], wv), ("device", h, w, gap, E)
            assert (g[:, :, 3:] == FILL).all()
        assert np.array_equal(read(d_y, np.uint8, ybuf.shape), ybuf) and np.array_equal(read(d_uv, np.uint8, uvbuf.shape), uvbuf)


# ----------------------------------------------------------------------------- 2. the frame
_SEQ = {}


def _pair_sequence(n=6):
    """n full-resolution pairs (H x W per eye) of one scene in which a flat rectangle moves 8 px per frame over both eyes, under fresh
    noise of +-2 per channel (test_temporal_ref.mixed_sequence at this size): in every frame the colour gate of the temporal step
    is closed where the rectangle was or is and open elsewhere; the rectangle's disparity alternates between -3 and -5, one pixel
    from the background's, so inside the closed gate the two frames' maps differ by less than the disparity gate: the step's result
    depends on the PREVIOUS frame's images"""
    from stm_amd import synth
    if n not in _SEQ:
        L, R, _ = synth.stereo_pair(H, W, D, ZD)
        rng = np.random.RandomState(11)
        seq = []
        for k in range(n):
            pair = []
            for v, x0 in ((L, 6 + 8 * k), (R, 6 + 8 * k - (3 if k % 2 == 0 else 5))):  # one pixel either side of the background's -4
                v = v.copy()
                v[10:24, x0:x0 + 14] = (200, 60, 30)
                pair.append(np.clip(v.astype(np.int32) + rng.randint(-2, 3, size=v.shape), 0, 255).astype(np.uint8))
            seq.append(tuple(pair))
        for a in [v for pair in seq for v in pair]:
            a.setflags(write=False)
        _SEQ[n] = seq
    return _SEQ[n]


def _eyes(sbs):
    return sbs[:, :W], sbs[:, W:]


def _history_matters(cur_maps, prev_maps, sbs, sbs_prev, want_maps):
    """The inputs of one temporal step, all unpacked: the colour gate both passes and fails in each eye; the numpy statement on them
    gives want_maps; and the same statement with a WRONG history image (this frame's own: what a call that never unpacked the
    previous packed frame, or unpacked the wrong buffer, would see) gives something else -- so a comparison with want_maps
    sees the history images"""
    for v in (0, 1):
        img, img_prev = _eyes(sbs)[v], _eyes(sbs_prev)[v]
        m = sad_max(img, img_prev)
        assert (m <= THRESH_COLOR).any() and (m > THRESH_COLOR).any(), v
        assert np.array_equal(temporal_ref(cur_maps[v], prev_maps[v], img, img_prev), want_maps[v]), v
        assert not np.array_equal(temporal_ref(cur_maps[v], prev_maps[v], img, img), want_maps[v]), v
        assert not np.array_equal(want_maps[v], cur_maps[v]), v  # the step did something


_PACKED = {}


def _packed_sequence(setting, fmt):
    """the sequence packed under `setting` (gap _gap(setting), noise-free fill 0x33 in the gap), as BGR frames or NV12 plane pairs,
    with the unpacked side-by-side BGR frames the numpy statement gives; computed once, read only"""
    from stm_amd import synth
    key = (setting, fmt)
    if key not in _PACKED:
        gap = _gap(setting)
        frames, sbs = [], []
        for L, R in _pair_sequence():
            f = synth.pack_frame(L, R, setting[0], setting[1], gap, fill=0x33)
            if fmt == "nv12":
                y, uv = synth.bgr_to_nv12(f, 0)
                frames.append((y, uv))
                sbs.append(np.ascontiguousarray(np.concatenate(unpack_nv12_ref(y, uv, H, W, setting, gap, 0), axis=1)))
            else:
                frames.append(f)
                sbs.append(unpacked_sbs(f, H, W, setting, gap))
        for a in sbs + [x for f in frames for x in (f if isinstance(f, tuple) else (f,))]:
            a.setflags(write=False)
        _PACKED[key] = (frames, sbs, (setting[0], setting[1], setting[2], gap))
    return _PACKED[key]


def _outputs(fill=0):
    import torch
    dl = torch.full((H, W), float(fill), dtype=torch.float32, device="cuda")
    return dl, torch.full_like(dl, float(fill)), torch.full((H, W, 3), fill, dtype=torch.uint8, device="cuda")


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _plain_call(sbs, p, stages, hist=None):
    """packing off: stm_d_adcensus_stm / stm_d_adcensus_stm_t on a side-by-side frame; hist = (prev sbs, prev dl, prev dr)"""
    import torch
    from stm_amd import device_api as dev
    assert dev.get_packing() == dev.PACKING_OFF
    dl, dr, out = _outputs()
    if stages & T:
        h = [None] * 3 if hist is None else [_cuda(a) for a in hist]
        dev.d_adcensus_stm_t(_cuda(sbs), dl, dr, out, p, stages, h[0], h[1], h[2], ALPHA, THRESH_COLOR, THRESH_DISP)
    else:
        dev.d_adcensus_stm(_cuda(sbs), dl, dr, out, p, stages=stages)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()


def _packed_call(frame, pk, p, stages, hist=None):
    """the same frame call under the packing pk.  frame: a BGR array or (y, uv); hist: BGR (prev packed frame, prev dl, prev dr),
    NV12 (prev img_l, prev img_r, prev dl, prev dr).  Returns (disp_l, disp_r, interlaced[, img_l, img_r])."""
    import torch
    from stm_amd import device_api as dev
    dl, dr, out = _outputs()
    dev.set_packing(*pk)
    try:
        if isinstance(frame, tuple):
            il = torch.full((H, W, 3), FILL, dtype=torch.uint8, device="cuda")
            ir = torch.full_like(il, FILL)
            h = [None] * 4 if hist is None else [_cuda(a) for a in hist]
            d_y, d_uv = _cuda(frame[0]), _cuda(frame[1])
            dev.d_adcensus_stm_nv12(d_y, d_uv, dl, dr, out, p, stages, 0, il, ir, h[0], h[1], h[2], h[3], ALPHA, THRESH_COLOR, THRESH_DISP)
            torch.cuda.synchronize()
            assert np.array_equal(d_y.cpu().numpy(), frame[0]) and np.array_equal(d_uv.cpu().numpy(), frame[1])  # read only
            return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy(), il.cpu().numpy(), ir.cpu().numpy()
        d_f = _cuda(frame)
        if stages & T:
            h = [None] * 3 if hist is None else [_cuda(a) for a in hist]
            dev.d_adcensus_stm_t(d_f, dl, dr, out, p, stages, h[0], h[1], h[2], ALPHA, THRESH_COLOR, THRESH_DISP)
        else:
            dev.d_adcensus_stm(d_f, dl, dr, out, p, stages=stages)
        torch.cuda.synchronize()
        assert np.array_equal(d_f.cpu().numpy(), frame)
        return dl.cpu().numpy(), dr.cpu().numpy(), out.cpu().numpy()
    finally:
        dev.set_packing(0, 0, 0, 0)


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
def test_frame_equals_the_frame_on_the_unpacked_pair(gpu_ready, setting, fmt):
    """36 x 132, D = 16: stages 3, 3 | 0x200 | 0x400 | 0x800, and 2 | 0x2000 with the previous frame as history"""
    p = _params()
    frames, sbs, pk = _packed_sequence(setting, fmt)
    for stages in (3, 3 | SUBPIXEL | INTERP | LINEAR_WARP):
        got = _packed_call(frames[1], pk, p, stages)
        want = _plain_call(sbs[1], p, stages)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), (stages, k)
        assert want[0].any() and want[2].any()
        if fmt == "nv12":  # the split images the call hands out are the unpacked eyes
            assert np.array_equal(got[3], sbs[1][:, :W]) and np.array_equal(got[4], sbs[1][:, W:])
    # the history maps: frame 0's, moved by a quarter pixel so that every pixel whose two gates are open changes
    first = _plain_call(sbs[0], p, 2)
    ql, qr = first[0] + np.float32(0.25), first[1] - np.float32(0.25)
    want = _plain_call(sbs[1], p, 2 | T, (sbs[0], ql, qr))
    _history_matters(_plain_call(sbs[1], p, 2)[:2], (ql, qr), sbs[1], sbs[0], want[:2])
    hist = (sbs[0][:, :W], sbs[0][:, W:], ql, qr) if fmt == "nv12" else (frames[0], ql, qr)
    got = _packed_call(frames[1], pk, p, 2 | T, hist)
    for k in range(3):
        assert np.array_equal(got[k], want[k]), ("temporal", k)
    # a first frame (all history pointers null) is the call without the bit
    a, b = _packed_call(frames[1], pk, p, 2 | T), _packed_call(frames[1], pk, p, 2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_fused_against_plain(gpu_ready, stm, fmt):
    """stm_k_front_pack (variant 0) against the stage kernel followed by the unfused kernels (variant 600)"""
    p = _params()
    lib = stm.lib()
    for setting in ((1, 1, 1), (3, 0, 0), (2, 1, 0)):
        frames, sbs, pk = _packed_sequence(setting, fmt)
        a = _packed_call(frames[2], pk, p, 3)
        try:
            lib.stm_set_agg_variant(600)
            b = _packed_call(frames[2], pk, p, 3)
        finally:
            lib.stm_set_agg_variant(0)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), setting


def test_four_byte_pixels_and_odd_addresses(gpu_ready, stm):
    """the frame under packing 1 with elem_sz 4, a row longer than the rule, every buffer at an odd address inside one arena: maps
    against the call on the unpacked 3-byte frame, the guard bands and the frame stay"""
    import torch
    from test_gpu_caller_buffers import Arena, P, read
    from stm_amd import synth
    p = _params()
    lib = stm.lib()
    lib.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    setting, gap = (1, 1, 1), 6
    L, R = _pair_sequence()[3]
    f3 = synth.pack_frame(L, R, 1, 1, gap, extra_cols=3, fill=0x33)
    frame = np.full(f3.shape[:2] + (4,), 0xC3, np.uint8)
    frame[:, :, :3] = f3
    want = _plain_call(unpacked_sbs(f3, H, W, setting, gap), p, 3)
    arena = Arena(True, nbytes=1 << 20)
    d_f = arena.put(frame, 1)
    d_dl, d_dr = arena.put(np.zeros((H, W), np.float32), 4), arena.put(np.zeros((H, W), np.float32), 12)
    d_out = arena.put(np.full((H, W, 4), FILL, np.uint8), 9)
    assert lib.stm_set_packing(1, 1, 1, gap) == 0
    try:
        lib.stm_d_adcensus_stm(P(d_f), P(d_dl), P(d_dr), P(d_out), H, frame.shape[1], W, H, W, 4, p.num_views, p.angle, p.num_disp, p.zero_disp,
                               p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, 3)
    finally:
        lib.stm_set_packing(0, 0, 0, 0)
    assert arena.intact()
    assert np.array_equal(read(d_f, np.uint8, frame.shape), frame)
    assert np.array_equal(read(d_dl, np.float32, (H, W)), want[0]) and np.array_equal(read(d_dr, np.float32, (H, W)), want[1])
    out = read(d_out, np.uint8, (H, W, 4))
    assert (out[:, :, 3] == FILL).all() and out[:, :, :3].any()


def test_packing_off_is_the_call_without_it(gpu_ready):
    """(0, 0, 0, 0) set explicitly against a thread that never called stm_set_packing: bit-identical frames"""
    p = _params()
    sbs = _packed_sequence((0, 0, 0), "bgr")[1][1]
    res = {}

    def run(name, explicit):
        import torch
        from stm_amd import device_api as dev
        torch.cuda.set_device(0)
        if explicit:
            dev.set_packing(0, 0, 0, 0)
        res[name] = _plain_call(sbs, p, 3 | SUBPIXEL | INTERP)

    for name, explicit in (("untouched", False), ("explicit", True)):
        t = threading.Thread(target=run, args=(name, explicit))
        t.start()
        t.join()
    assert set(res) == {"untouched", "explicit"}
    assert all(np.array_equal(a, b) for a, b in zip(res["untouched"], res["explicit"]))
    assert res["explicit"][0].any() and res["explicit"][2].any()


# ----------------------------------------------------------------------------- 3. the stream
def _stream(frames, p, stages, fmt, packing=None, inplace=False):
    from stm_amd import video
    fs = video.FrameStream(H, W, p, stages=stages, input_format=fmt, packing=packing)
    try:
        got, pending = [], 0
        for f in frames:
            if pending == 2:
                got.append(fs.collect())
                pending -= 1
            if inplace:
                buf = fs.input_buffer()
                assert buf is not None and buf.shape == f.shape
                buf[...] = f
                assert fs.submit_inplace() >= 0
            else:
                assert fs.submit(f) >= 0
            pending += 1
        while pending:
            got.append(fs.collect())
            pending -= 1
    finally:
        fs.close()
    assert [g[0] for g in got] == list(range(len(frames)))
    return got


@pytest.mark.parametrize("stages", [3, 3 | T], ids=["0x3", "0x2003"])
@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
@pytest.mark.parametrize("setting", [(1, 0, 1), (1, 1, 1), (2, 0, 0), (3, 1, 0)], ids=lambda s: "p%d_s%d_f%d" % s)
def test_stream_under_a_packing(gpu_ready, setting, fmt, stages):
    """six packed frames, two in flight, so both slots replay their captured graph: every collected frame equals the one of a
    stream, packing off, fed the unpacked frames; with 0x2000 at the stream's default thresholds"""
    from stm_amd import device_api as dev
    p = _params()
    frames, sbs, pk = _packed_sequence(setting, fmt)
    feed = [nv12_frame(y, uv) for y, uv in frames] if fmt == "nv12" else frames
    got = _stream(feed, p, stages, fmt, pk, inplace=(setting[1] == 1))
    assert dev.get_packing() == dev.PACKING_OFF
    want = _stream(sbs, p, stages, "bgr")
    for k in range(6):
        for j in range(1, 4):
            assert np.array_equal(got[k][j], want[k][j]), (k, j)
    assert want[5][1].any() and want[5][3].any()
    if stages & T:  # every frame but the first, the replayed ones included, depends on the previous frame's unpacked images
        for k in range(1, 6):
            _history_matters(_plain_call(sbs[k], p, 3)[:2], want[k - 1][1:3], sbs[k], sbs[k - 1], want[k][1:3])


def test_stream_keeps_its_own_packing(gpu_ready):
    """the calling thread's packing does not reach a stream's frames, and the stream's does not leak out"""
    from stm_amd import device_api as dev
    p = _params()
    frames, sbs, pk = _packed_sequence((1, 0, 0), "bgr")
    dev.set_packing(2, 1, 0, 4)
    try:
        got = _stream(frames[:3], p, 3, "bgr", pk)
        plain = _stream(sbs[:3], p, 3, "bgr")
        assert dev.get_packing() == (2, 1, 0, 4)
    finally:
        dev.set_packing(0, 0, 0, 0)
    for k in range(3):
        want = _plain_call(sbs[k], p, 3)
        for j in range(3):
            assert np.array_equal(got[k][1 + j], want[j]) and np.array_equal(plain[k][1 + j], want[j]), (k, j)


def test_stream_set_packing_rules(gpu_ready):
    from stm_amd import device_api as dev, video
    lib = dev.lib()
    p = _params()
    frames, _, pk = _packed_sequence((3, 1, 1), "nv12")
    lib.stm_set_error_mode(1)
    try:
        fs = video.FrameStream(H, W, p)  # num_cols_sbs = 2 W
        try:
            for args, word in (((4, 0, 0, 0), b"packing"), ((0, 2, 0, 0), b"swap"), ((1, 0, 2, 0), b"filter"), ((0, 0, 1, 0), b"filter"),
                               ((0, 0, 0, -1), b"gap"), ((0, 0, 0, 2), b"num_cols_sbs")):
                assert lib.stm_stream_set_packing(fs._h, *args) == -1
                err = lib.stm_last_error()
                assert b"stream_set_packing" in err and word in err, (args, err)
            with pytest.raises(ValueError):
                fs.set_packing(0, 0, 0, 2)
            assert fs.in_shape == (H, 2 * W, 3)
            # either order: NV12 first, then a packing whose evenness rule the geometry breaks (gap odd) and one it keeps
            fs.set_input("nv12", 0)
            assert lib.stm_stream_set_packing(fs._h, 2, 0, 0, 3) == -1 and b"gap" in lib.stm_last_error()
            fs.set_packing(2, 1, 0, 4)
            assert fs.in_shape == ((2 * H + 4) * 3 // 2, 2 * W) and fs.input_buffer().shape == fs.in_shape
            fs.set_packing(0, 0, 0, 0)
            assert fs.in_shape == (H * 3 // 2, 2 * W) and fs.input_buffer().shape == fs.in_shape
        finally:
            fs.close()
        # the other order: the packing first, NV12 second checks the combination
        fs = video.FrameStream(H, W, p, packing=(2, 0, 0, 3))
        try:
            with pytest.raises(ValueError):
                fs.set_input("nv12", 0)
            assert b"stream_set_input" in lib.stm_last_error() and b"gap" in lib.stm_last_error()
        finally:
            fs.close()
        fs = video.FrameStream(H, W, p, input_format="nv12", packing=pk)
        try:
            assert fs.submit(nv12_frame(*frames[0])) == 0
            assert lib.stm_stream_set_packing(fs._h, 0, 0, 0, 0) == -1
            err = lib.stm_last_error()
            assert b"stream_set_packing" in err and b"first submit" in err, err
            assert lib.stm_stream_set_stages(fs._h, 3 | 0x4000) == -1  # an input geometry, not a stage bit
            assert fs.collect()[0] == 0
        finally:
            fs.close()
    finally:
        lib.stm_set_error_mode(0)


# ----------------------------------------------------------------------------- the video driver
def test_video_cli_with_packing(gpu_ready, tmp_path):
    """tools/stm_video.py --packing P SWAP FILTER GAP on a directory of packed BMP frames: what it writes are the per-frame calls'"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from stm_amd import bmp_io, device_api as dev
    frames, sbs, pk = _packed_sequence((1, 1, 1), "bgr")
    src = tmp_path / "in"
    src.mkdir()
    for k in range(3):
        bmp_io.write_bmp(str(src / ("f_%03d.bmp" % k)), frames[k])
    out = tmp_path / "o"
    args = [sys.executable, os.path.join(ROOT, "tools", "stm_video.py"), str(src), "8", "18.43", str(W), str(H), str(D), str(ZD),
            "10", "30", "6", "20", "17", "8", "20", "0.4", str(out), "--packing"] + [str(v) for v in pk]
    subprocess.check_call(args)
    p = dev.FrameParams(num_disp=D, zero_disp=ZD, usd=17, lsd=8, angle=18.0)  # the tool truncates the slant
    for k in range(3):
        want = _plain_call(sbs[k], p, 3)
        assert np.array_equal(bmp_io.read_bmp(str(out / ("interlaced_%05d.bmp" % k))), want[2]), k
    assert subprocess.call(args[:17] + ["--packing", "1", "0"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0
