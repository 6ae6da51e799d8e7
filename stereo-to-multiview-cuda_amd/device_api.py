"""Device-flavour stage API: torch CUDA(=HIP) tensors in, work enqueued on torch's current stream,
nothing synchronised -- the analogue of the reference's `d_stage(device ptrs...)` wrappers that
adcensus_stm (d_io.cu:7-238) chains.  torch is plumbing only (device memory + streams); every kernel is
hand-written HIP inside libstm_hip.so.
"""
import ctypes as C

import torch

from ._lib import f32p, f32pp, lib


def _use_current_stream():
    lib().stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _p(t):
    return C.c_void_p(t.data_ptr())


# d_adcensus_stm `stages` bit: sub-pixel enhancement of the whole-pixel maps (not together with 0x100, HSLO)
STAGE_SUBPIXEL = 0x200
# ... outlier interpolation after region voting (stages 2 and 3 only; combines with 0x100 and with STAGE_SUBPIXEL)
STAGE_INTERP = 0x400
# ... the views of stage 3 rendered at the fractional warp coordinate (stm_dibr_dbm_lin; stage 3 only, combines with every other bit)
STAGE_LINEAR_WARP = 0x800
# d_adcensus_stm_2s only: the disparity maps scaled up by the guided up-sampler (stm_disp_upsample) instead of the bilinear blend
STAGE_GUIDED_UP = 0x1000
# d_adcensus_stm_t and the frame stream only: the filtered maps stabilised against the previous frame's (stm_disp_temporal)
STAGE_TEMPORAL = 0x2000
TEMPORAL_DEFAULTS = (0.5, 24, 1.5)  # alpha, thresh_color, thresh_disp of a frame sequence


class FrameParams:
    """Parameters of one adcensus_stm call (d_io.h:32-40), defaults from SURVEY.md section 8d."""

    def __init__(self, num_disp=64, zero_disp=32, num_views=8, angle=18.43, ad_coeff=10.0, census_coeff=30.0,
                 ucd=6.0, lcd=20.0, usd=34, lsd=17, thresh_s=20, thresh_h=0.4, out_rows=None, out_cols=None):
        self.num_disp, self.zero_disp, self.num_views, self.angle = num_disp, zero_disp, num_views, angle
        self.ad_coeff, self.census_coeff = ad_coeff, census_coeff
        self.ucd, self.lcd, self.usd, self.lsd = ucd, lcd, usd, lsd
        self.thresh_s, self.thresh_h = thresh_s, thresh_h
        self.out_rows, self.out_cols = out_rows, out_cols


# stm_agg_path's bit field
AGG_MATRIX_PIPE, AGG_PX, AGG_VREGS, AGG_HREGS, AGG_SPLIT = 1, 2, 4, 8, 1 << 16


def agg_path(num_disp, zero_disp, num_rows, num_cols, usd, stages=3):
    """stm_agg_path: which aggregation kernels a frame call with these arguments takes under the current stm_set_agg_variant, as a
    bit field (AGG_*; bits 8..15 = agg_path_waves).  Host arithmetic only: it launches nothing and needs no GPU."""
    return int(lib().stm_agg_path(int(num_disp), int(zero_disp), int(num_rows), int(num_cols), int(usd), int(stages)))


def agg_path_waves(path):
    """waves per block of the cost-fusing first pass in an agg_path value: 12, 8, or 0 when another kernel runs"""
    return (int(path) >> 8) & 0xff


def first_pass_path(num_disp, zero_disp, num_rows, num_cols, usd, stages=3):
    """stm_first_pass_path: 0 when stm_k_pq_hc (or another kernel) runs the first horizontal pass of such a frame call under the
    current stm_set_agg_variant, else the blocks per image row of stm_k_pq_hc2, which sweeps both views from one ring of costs.
    Host arithmetic only: it launches nothing and needs no GPU."""
    return int(lib().stm_first_pass_path(int(num_disp), int(zero_disp), int(num_rows), int(num_cols), int(usd), int(stages)))


def px_order(num_disp, zero_disp, num_rows, num_cols, usd, stages=3):
    """stm_px_order: -1 where such a frame call is off the pixel-major (PX) volumes under the current stm_set_agg_variant, else the
    order of the hypotheses inside a pixel's record as the last pass reads it: 2 = after the 16-byte stores of the first pass and
    of the vertical kernel (the default), 0 = ascending, with their 4-byte stores (variant 2000000000).  Host arithmetic only: it launches nothing and needs no GPU."""
    return int(lib().stm_px_order(int(num_disp), int(zero_disp), int(num_rows), int(num_cols), int(usd), int(stages)))


# stm_irv_path's bit field
IRV_PRUNE, IRV_RUNS, IRV_CHAIN = 1, 2, 4


def irv_path(num_rows, num_cols, usd, iterations=5, device_flavour=True, with_dcc=False):
    """stm_irv_path: which region-voting kernels a call with these arguments takes under the current stm_set_agg_variant,
    stm_set_irv_paper_ratio and stm_set_irv_chunk, as a bit field (IRV_*; irv_path_tile_sh, irv_path_chunk).  with_dcc: a frame
    call; otherwise d_dr_irv (device_flavour) or dr_irv.  Host arithmetic only: it launches nothing and needs no GPU."""
    return int(lib().stm_irv_path(int(num_rows), int(num_cols), int(usd), int(iterations), int(bool(device_flavour)), int(bool(with_dcc))))


def irv_path_tile_sh(path):
    """log2 of the dirty tiles' edge in an irv_path value"""
    return (int(path) >> 8) & 0xf


def irv_path_chunk(path):
    """the forced entries per trip in an irv_path value, 0 = the kernel's own rule"""
    return (int(path) >> 16) & 0x1f


def set_irv_chunk(entries=0):
    """stm_set_irv_chunk: list entries per wave and trip of the column-run vote kernel; 0 = the kernel's own rule (the default),
    1 .. 16 = forced.  Raises ValueError where the library refuses (the setting then stays as it was) -- under stm_set_error_mode(1);
    in the default error mode 0 the library exits, like on any error."""
    if int(lib().stm_set_irv_chunk(int(entries))) != 0:
        raise ValueError("stm_set_irv_chunk(%d) refused: %s" % (entries, lib().stm_last_error().decode()))


def set_agg_tap(h1=None, v2=None, h4=None, inject_v2=None):
    """stm_set_agg_tap: test access to the aggregation chain of this thread's frame calls.  Each argument is None or a contiguous
    float32 tensor [2][D][H][W] on the GPU (view, true hypothesis, the size the pair is matched at): h1 / v2 receive the volume after
    the first horizontal pass / after both vertical passes, inject_v2 is written over V2 before the last pass, h4 receives the last
    pass's output where the chain keeps it (stage bit 0x100).  All None = off.  The caller keeps the tensors alive while the tap is
    set (agg_tap does both).  Raises ValueError where the library refuses."""
    for t in (h1, v2, h4, inject_v2):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4 and t.shape[0] == 2)
    if int(lib().stm_set_agg_tap(*[_p(t) if t is not None else None for t in (h1, v2, h4, inject_v2)])) != 0:
        raise ValueError("stm_set_agg_tap refused: %s" % lib().stm_last_error().decode())


class agg_tap:
    """`with agg_tap(h1=..., v2=..., h4=..., inject_v2=...):` -- set_agg_tap around a block of frame calls; the tap is always cleared
    on the way out, and the tensors stay referenced until then."""

    def __init__(self, h1=None, v2=None, h4=None, inject_v2=None):
        self.bufs = (h1, v2, h4, inject_v2)

    def __enter__(self):
        set_agg_tap(*self.bufs)
        return self

    def __exit__(self, *exc):
        set_agg_tap()
        return False


def set_hslo_tap(s2=None, s3=None, fin=None):
    """stm_set_hslo_tap (include/stm_hslo_tap.h): test access to the scanline passes of this thread's calls.  Each argument is None or
    a contiguous float32 tensor [views][D][H][W] on the GPU -- views = 1 for the stage calls, 2 (left, right) for a frame call with
    stage bit 0x100: s2 receives C_lr + C_rl, s3 that + C_tb, fin the final volume ((s3 + C_bt) * 0.25).  All None = off.  The caller
    keeps the tensors alive while the tap is set (hslo_tap does both).  Raises ValueError where the library refuses."""
    for t in (s2, s3, fin):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4 and t.shape[0] in (1, 2))
    if int(lib().stm_set_hslo_tap(*[_p(t) if t is not None else None for t in (s2, s3, fin)])) != 0:
        raise ValueError("stm_set_hslo_tap refused: %s" % lib().stm_last_error().decode())


class hslo_tap:
    """`with hslo_tap(s2=..., s3=..., fin=...):` -- set_hslo_tap around a block of calls; the tap is always cleared on the way out,
    and the tensors stay referenced until then."""

    def __init__(self, s2=None, s3=None, fin=None):
        self.bufs = (s2, s3, fin)

    def __enter__(self):
        set_hslo_tap(*self.bufs)
        return self

    def __exit__(self, *exc):
        set_hslo_tap()
        return False


def set_lens(mode, pitch=0.0, slope=0.0, centre=0.0):
    """stm_set_lens: the calling thread's display geometry, which every rendering frame call interlaces through.  mode 0 = off (the
    reference's interlacer, the default), 1 = nearest view, 2 = two views blended, 3 = every sub-pixel rendered at its own
    continuous position; pitch in sub-pixels per lens (>= 1), slope in sub-pixels per output row, centre in lenses.  Raises
    ValueError where the library refuses (it returns -1; in error mode 0 it exits like any error)."""
    if int(lib().stm_set_lens(int(mode), float(pitch), float(slope), float(centre))) != 0:
        raise ValueError("stm_set_lens(%d, %g, %g, %g) refused: %s" % (mode, pitch, slope, centre, lib().stm_last_error().decode()))


def set_layout(layout=0, tiles_x=1, tiles_y=1, order=0, filter=0):
    """stm_set_layout: the calling thread's output geometry, which every rendering frame call writes.  layout 0 = the interlaced
    frame (the default; the other arguments are ignored), 1 = a quilt of tiles_x x tiles_y tiles, one whole view each (tiles_x *
    tiles_y must equal the frame's num_views); order bit 0 = tile rows bottom-up, bit 1 = view order reversed (tile 0 = the
    leftmost camera); filter 0 = the reference's four-neighbour sampler, 1 = the area average.  Raises ValueError where the
    library refuses."""
    if int(lib().stm_set_layout(int(layout), int(tiles_x), int(tiles_y), int(order), int(filter))) != 0:
        raise ValueError("stm_set_layout(%d, %d, %d, %d, %d) refused: %s"
                         % (layout, tiles_x, tiles_y, order, filter, lib().stm_last_error().decode()))


def get_layout():
    """stm_get_layout: the calling thread's (layout, tiles_x, tiles_y, order, filter) as the library holds it"""
    out = (C.c_int * 5)()
    lib().stm_get_layout(out)
    return tuple(int(v) for v in out)


def set_output(format=0, matrix=0, pitch=0, uv_row=0):
    """stm_set_output: the calling thread's output format, which every rendering frame call writes.  format 0 = BGR (the default; the
    other arguments are ignored), 1 = NV12 (quilts only): the frame calls' `interlaced` is then ONE surface, a 2-D uint8 tensor of
    (R + Hout / 2) x P -- the Y plane in rows 0 .. Hout - 1, the interleaved UV plane from row R; P = pitch or Wout, R = uv_row or
    Hout -- converted by `matrix` (0 / 1 = BT.601 / BT.709 limited range, 2 / 3 = full range).  Raises ValueError where the library
    refuses."""
    if int(lib().stm_set_output(int(format), int(matrix), int(pitch), int(uv_row))) != 0:
        raise ValueError("stm_set_output(%d, %d, %d, %d) refused: %s" % (format, matrix, pitch, uv_row, lib().stm_last_error().decode()))


def get_output():
    """stm_get_output: the calling thread's (format, matrix, pitch, uv_row) as the library holds it"""
    out = (C.c_int * 4)()
    lib().stm_get_output(out)
    return tuple(int(v) for v in out)


_overlay_keepalive = {}  # thread id -> the tensor the library's setting of that thread points into


def _check_overlay(overlay):
    assert overlay.is_cuda and overlay.dtype == torch.uint8 and overlay.is_contiguous()
    assert overlay.dim() == 3 and overlay.shape[2] == 4, "an overlay is uint8 [rows][cols][4]: B, G, R, A, premultiplied"


def set_overlay(d_overlay, x0=0, y0=0, disparity=0.0):
    """stm_set_overlay: the calling thread's overlay, which every rendering frame call composites into its finished frame as its
    last launch (include/stm_hip.h, stm_mux_overlay).  d_overlay: a uint8 [rows][cols][4] tensor on the GPU -- B, G, R, A with
    premultiplied alpha (video.premultiply converts straight alpha) -- or None = off, the default.  (x0, y0): the view pixel its
    top-left corner sits at -- a pixel of the frame, or of one tile of a quilt; disparity: end to end in the maps' sign convention,
    > 0 behind the screen, < 0 in front, 0 on it.  The tensor is kept alive here until the setting changes; its contents must not
    change while a frame call may read it.  Raises ValueError where the library refuses."""
    import threading
    if d_overlay is None:
        lib().stm_set_overlay(0, None, 0, 0, 0, 0, 0.0)
        _overlay_keepalive.pop(threading.get_ident(), None)
        return
    _check_overlay(d_overlay)
    if int(lib().stm_set_overlay(1, _p(d_overlay), d_overlay.shape[0], d_overlay.shape[1], int(x0), int(y0), float(disparity))) != 0:
        raise ValueError("stm_set_overlay(%d x %d at (%d, %d), disparity %g) refused: %s"
                         % (d_overlay.shape[0], d_overlay.shape[1], x0, y0, disparity, lib().stm_last_error().decode()))
    _overlay_keepalive[threading.get_ident()] = d_overlay


OVERLAY_AUTO_DEFAULTS = (20, 1.0, 8, 1.0, 0.1)  # near_permille, margin, pad, rate_near, rate_far: choices, not measurements


def set_overlay_auto(limit_lo=None, limit_hi=None, near_permille=20, margin=1.0, pad=8, rate_near=1.0, rate_far=0.1, state=None):
    """stm_set_overlay_auto: the calling thread's automatic overlay placement.  While it is on and the thread's overlay is on
    (set_overlay, whose disparity is then ignored), every rendering frame call fits the overlay's disparity to the maps under the
    overlay's alpha box on the GPU (d_overlay_fit has the parameters) and composites at fminf(fmaxf(state[1], limit_lo), limit_hi).
    `state`: a float32 tensor of four elements on the GPU, {valid, disparity, nearest, 0}, which carries the history from frame to
    frame (zero `valid` to reset it) -- the caller keeps it alive while the setting is in use; None = every frame on its own.
    limit_lo None switches the setting off.  Raises ValueError where the library refuses."""
    if limit_lo is None:
        lib().stm_set_overlay_auto(0, 0, 0.0, 0, 0.0, 0.0, 0.0, 0.0, None)
        return
    if state is not None:
        assert state.is_cuda and state.dtype == torch.float32 and state.is_contiguous() and state.numel() == 4
    if int(lib().stm_set_overlay_auto(1, int(near_permille), float(margin), int(pad), float(limit_lo), float(limit_hi), float(rate_near),
                                      float(rate_far), _p(state) if state is not None else None)) != 0:
        raise ValueError("stm_set_overlay_auto(%d, %g, %d, %g, %g, %g, %g) refused: %s"
                         % (near_permille, margin, pad, limit_lo, limit_hi, rate_near, rate_far, lib().stm_last_error().decode()))


def get_overlay_auto():
    """stm_get_overlay_auto: the calling thread's (mode, near_permille, margin, pad, limit_lo, limit_hi, rate_near, rate_far)"""
    m = (C.c_int * 3)()
    v = (C.c_float * 5)()
    lib().stm_get_overlay_auto(m, C.cast(v, f32p))
    return (m[0], m[1], v[0], m[2], v[1], v[2], v[3], v[4])


def d_overlay_fit(disp_l, disp_r, overlay, x0, y0, view_rows, view_cols, limit_lo, limit_hi, state, gain=1.0, conv=0.0, near_permille=20,
                  margin=1.0, pad=8, rate_near=1.0, rate_far=0.1, restart=False, cut_state=None):
    """stm_d_overlay_fit: the measurement of the overlay's placement as a stage -- the alpha box of `overlay` (uint8 [rows][cols][4]
    on the GPU) at (x0, y0) of the view view_rows x view_cols, both maps (float32 [H][W] on the GPU) under its footprint widened by
    `pad` into the quarter-pixel histogram, the near_permille percentile mapped through the budget (gain, conv) and the view's
    width, `margin` subtracted, clamped to [limit_lo, limit_hi], and the update of `state` (float32, four elements on the GPU:
    valid, disparity, nearest, 0) in place at rate_near / rate_far; cut_state: stm_cut_detect's 260 ints on the GPU or None.
    Nothing is synchronised."""
    H, W = disp_l.shape
    for t in (disp_l, disp_r):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (H, W)
    _check_overlay(overlay)
    assert state.is_cuda and state.dtype == torch.float32 and state.is_contiguous() and state.numel() == 4
    if cut_state is not None:
        assert cut_state.is_cuda and cut_state.dtype == torch.int32 and cut_state.is_contiguous() and cut_state.numel() >= 2
    _use_current_stream()
    lib().stm_d_overlay_fit(_p(disp_l), _p(disp_r), H, W, _p(overlay), overlay.shape[0], overlay.shape[1], int(x0), int(y0), int(view_rows),
                            int(view_cols), float(gain), float(conv), int(near_permille), float(margin), int(pad), float(limit_lo),
                            float(limit_hi), float(rate_near), float(rate_far), int(bool(restart)), _p(state),
                            _p(cut_state) if cut_state is not None else None)


def get_overlay():
    """stm_get_overlay: the calling thread's (mode, ov_rows, ov_cols, x0, y0, disparity) as the library holds it"""
    out = (C.c_int * 5)()
    disp = C.c_float(0.0)
    lib().stm_get_overlay(out, C.cast(C.byref(disp), f32p))
    return tuple(int(v) for v in out) + (float(disp.value),)


def d_mux_overlay(frame, overlay, x0, y0, disparity, num_views, angle=18.43, lens=None, layout=None):
    """stm_d_mux_overlay: the overlay (uint8 [rows][cols][4] on the GPU, premultiplied B, G, R, A) composited in place into the
    finished frame (uint8 [Ho][Wo][E] on the GPU; only bytes 0 .. 2 of the pixels inside the overlay's bounding box are written).
    lens = (mode, pitch, slope, centre) as set_lens, None = the reference's interlacer at `angle`; layout = (1, tiles_x, tiles_y,
    order) for a quilt, None = the interlaced frame."""
    assert frame.is_cuda and frame.dtype == torch.uint8 and frame.dim() == 3 and frame.is_contiguous()
    _check_overlay(overlay)
    ln = tuple(lens) if lens is not None else (0, 0.0, 0.0, 0.0)
    lo = tuple(layout)[:4] if layout is not None else (0, 1, 1, 0)
    _use_current_stream()
    lib().stm_d_mux_overlay(_p(frame), _p(overlay), overlay.shape[0], overlay.shape[1], int(x0), int(y0), float(disparity),
                            int(num_views), float(angle), int(ln[0]), float(ln[1]), float(ln[2]), float(ln[3]), int(lo[0]), int(lo[1]),
                            int(lo[2]), int(lo[3]), frame.shape[0], frame.shape[1], frame.shape[2])


def _out_size(interlaced, p):
    """(Hout, Wout) of a frame call's output: a BGR frame's first two dimensions, or -- under set_output's format 1 -- what the 2-D
    surface of (R + Hout / 2) x P holds; p.out_rows / p.out_cols, where set, say it outright (needed with a pitch beyond Wout)"""
    fmt, _, pitch, uv_row = get_output()
    if fmt == 0:
        return interlaced.shape[0], interlaced.shape[1]
    assert interlaced.dim() == 2 and interlaced.dtype == torch.uint8 and interlaced.is_contiguous()
    rows, P = interlaced.shape
    assert pitch in (0, P), "the surface's row length must be the pitch of set_output"
    Wo = p.out_cols or P
    Ho = p.out_rows or ((rows - uv_row) * 2 if uv_row else rows * 2 // 3)
    assert rows >= (uv_row or Ho) + Ho // 2
    return Ho, Wo


def d_mux_nv12(y, uv, img, matrix=0):
    """stm_d_mux_nv12: the BGR image img (uint8 [H][W][E], H and W even) converted into the NV12 planes y (uint8 [H][>= W]) and uv
    (uint8 [H / 2][>= W], U and V interleaved, each the mean of a 2 x 2 block), 2-D tensors whose row stride is the plane's pitch;
    only the samples are written.  matrix: 0 / 1 = BT.601 / BT.709 limited range, 2 / 3 = BT.601 / BT.709 full range."""
    assert img.is_cuda and img.dtype == torch.uint8 and img.is_contiguous() and img.dim() == 3
    H, W, E = img.shape
    for t in (y, uv):
        assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1) and t.shape[1] >= W
    assert y.shape[0] == H and uv.shape[0] * 2 == H
    _use_current_stream()
    lib().stm_d_mux_nv12(_p(y), y.stride(0), _p(uv), uv.stride(0), _p(img), H, W, E, int(matrix))


PACKING_OFF = (0, 0, 0, 0)

def set_packing(packing=0, swap=0, filter=0, gap=0):
    """stm_set_packing: where the two eyes lie in the frames this thread's d_adcensus_stm, d_adcensus_stm_t and d_adcensus_stm_nv12
    are given.  packing 0 / 1 = side by side full / half width, 2 / 3 = top and bottom full / half height; swap 1 = the right eye
    first; filter 0 = linear, 1 = Catmull-Rom (the expansion of packings 1 and 3); gap = pixels between the eyes along the packing
    axis.  (0, 0, 0, 0) = off, the default.  Under a packing the unpacked eye's size is taken from disp_l.  Raises ValueError where
    the library refuses."""
    if int(lib().stm_set_packing(int(packing), int(swap), int(filter), int(gap))) != 0:
        raise ValueError("stm_set_packing(%d, %d, %d, %d) refused: %s" % (packing, swap, filter, gap, lib().stm_last_error().decode()))


def get_packing():
    """stm_get_packing: the calling thread's (packing, swap, filter, gap) as the library holds it, whoever set it"""
    out = (C.c_int * 4)()
    lib().stm_get_packing(out)
    return tuple(int(v) for v in out)


def packed_frame_rows(num_rows, packing):
    """rows_f of stm_hip.h: the rows of a packed frame whose unpacked eyes have num_rows rows; packing = (packing, swap, filter, gap)"""
    pk, gap = int(packing[0]), int(packing[3])
    return 2 * num_rows + gap if pk == 2 else 2 * (num_rows // 2) + gap if pk == 3 else num_rows


def _eye_shape(frame_rows, Wsbs, disp_l):
    """(H, W) of a frame call: half the frame's columns with packing off, disp_l's shape (the unpacked eye) under a packing"""
    pk = get_packing()
    if pk == PACKING_OFF:
        return frame_rows, Wsbs // 2
    H, W = disp_l.shape
    if frame_rows < packed_frame_rows(H, pk):
        raise ValueError("a frame of %d rows cannot hold two eyes of %d rows under packing %r" % (frame_rows, H, pk))
    return H, W


def d_demux_packed(img_l, img_r, img, packing):
    """stm_d_demux_packed: the two unpacked eyes of the packed BGR frame img (uint8 [rows_f][Wsbs][E] on the GPU) into img_l / img_r
    (uint8 [H][W][E], only the first three bytes of a pixel are written); packing = (packing, swap, filter, gap)."""
    H, W, E = img_l.shape
    assert img.is_cuda and img.dtype == torch.uint8 and img.is_contiguous() and img.dim() == 3 and img.shape[2] == E
    for t in (img_l, img_r):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    pk, sw, fl, gap = (int(v) for v in packing)
    assert img.shape[0] >= packed_frame_rows(H, packing)
    _use_current_stream()
    lib().stm_d_demux_packed(_p(img_l), _p(img_r), _p(img), H, img.shape[1], W, E, pk, sw, fl, gap)


def d_demux_nv12_packed(img_l, img_r, y, uv, packing, matrix=0, num_cols_sbs=None):
    """stm_d_demux_nv12_packed: d_demux_packed on a packed NV12 frame (planes as for d_demux_nv12, rows_f and rows_f / 2 rows)."""
    for t in (y, uv):
        assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1)
    H, W, E = img_l.shape
    for t in (img_l, img_r):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    Wsbs = y.shape[1] if num_cols_sbs is None else num_cols_sbs
    assert y.shape[0] >= packed_frame_rows(H, packing) and uv.shape[0] * 2 == y.shape[0]
    assert y.shape[1] >= Wsbs and uv.shape[1] >= 2 * ((Wsbs + 1) // 2)
    pk, sw, fl, gap = (int(v) for v in packing)
    _use_current_stream()
    lib().stm_d_demux_nv12_packed(_p(img_l), _p(img_r), _p(y), y.stride(0), _p(uv), uv.stride(0), H, Wsbs, W, E, int(matrix), pk, sw, fl, gap)


DEPTH_AUTO_DEFAULTS = (1.0, 20, 1.0)  # max_gain, clip_permille, rate of stm_set_depth_auto


def set_depth(mode, gain=1.0, conv=0.0):
    """stm_set_depth: the calling thread's depth budget, which every rendering frame call samples through.  mode 0 = off (the views
    span the camera baseline, the default), 1 = manual: a scene point of disparity delta is shown with gain * delta - conv (conv in
    input-view pixels; gain > 1 extrapolates beyond the two cameras), 2 = automatic: gain and conv fitted to every frame's disparity
    range on the GPU with set_depth_auto's parameters.  Raises ValueError where the library refuses."""
    if int(lib().stm_set_depth(int(mode), float(gain), float(conv))) != 0:
        raise ValueError("stm_set_depth(%d, %g, %g) refused: %s" % (mode, gain, conv, lib().stm_last_error().decode()))


def set_depth_auto(disp_lo, disp_hi, max_gain=1.0, clip_permille=20, rate=1.0, state=None):
    """stm_set_depth_auto: mode 2's parameters -- the budget [disp_lo, disp_hi] of displayed disparity in input-view pixels, the
    gain's ceiling, the share (in 1/1000) of pixels ignored at either end of the frame's range, the rate at which gain and conv
    follow a frame's fit, and `state`: a float32 tensor of four elements on the GPU, {valid, gain, conv, 0}, which carries the
    history from frame to frame (zero `valid` to reset it) -- the caller keeps it alive while the setting is in use; None = every
    frame on its own.  Raises ValueError where the library refuses."""
    if state is not None:
        assert state.is_cuda and state.dtype == torch.float32 and state.is_contiguous() and state.numel() == 4
    if int(lib().stm_set_depth_auto(float(disp_lo), float(disp_hi), float(max_gain), int(clip_permille), float(rate),
                                    _p(state) if state is not None else None)) != 0:
        raise ValueError("stm_set_depth_auto(%g, %g, %g, %d, %g) refused: %s"
                         % (disp_lo, disp_hi, max_gain, clip_permille, rate, lib().stm_last_error().decode()))


def d_depth_fit(disp_l, disp_r, disp_lo, disp_hi, max_gain, clip_permille, rate, state):
    """stm_d_depth_fit: the measurement of the automatic depth budget as a stage -- both maps (float32 [H][W] on the GPU) into the
    quarter-pixel histogram, the fit, the update of `state` (float32, four elements on the GPU) in place; nothing synchronised."""
    H, W = disp_l.shape
    for t in (disp_l, disp_r):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (H, W)
    assert state.is_cuda and state.dtype == torch.float32 and state.is_contiguous() and state.numel() == 4
    _use_current_stream()
    lib().stm_d_depth_fit(_p(disp_l), _p(disp_r), H, W, float(disp_lo), float(disp_hi), float(max_gain), int(clip_permille), float(rate),
                          _p(state))


def set_antialias(mode, strength=1.0, max_radius=8, gate=1.0):
    """stm_set_antialias: the calling thread's view antialiasing.  mode 0 = off (the default), 1 = every rendering frame call
    filters both images by their own maps before it renders from them (d_view_prefilter's rule): a horizontal box of
    1 + strength * |displayed disparity| / (N - 1) pixels, at most max_radius (1 .. 16) pixels to a side, whose taps are used only
    where the map stays within `gate` of the pixel's own value.  Raises ValueError where the library refuses."""
    if int(lib().stm_set_antialias(int(mode), float(strength), int(max_radius), float(gate))) != 0:
        raise ValueError("stm_set_antialias(%d, %g, %d, %g) refused: %s" % (mode, strength, max_radius, gate, lib().stm_last_error().decode()))


def get_antialias():
    """stm_get_antialias: the calling thread's (mode, strength, max_radius, gate) as the library holds it"""
    m = (C.c_int * 2)()
    v = (C.c_float * 2)()
    lib().stm_get_antialias(m, C.cast(v, f32p))
    return int(m[0]), float(v[0]), int(m[1]), float(v[1])


def set_align(mode, a=0.0, b=0.0, c=0.0):
    """stm_set_align: the calling thread's vertical alignment of the pair, applied to every frame call's input ahead of the matcher.
    mode 0 = off (the default), 1 = manual: the right eye is sampled at row y + a + b u + c v (u, v from the frame's centre),
    2 = automatic: the field measured on every frame on the GPU with set_align_auto's parameters.  Raises ValueError where the
    library refuses."""
    if int(lib().stm_set_align(int(mode), float(a), float(b), float(c))) != 0:
        raise ValueError("stm_set_align(%d, %g, %g, %g) refused: %s" % (mode, a, b, c, lib().stm_last_error().decode()))


def set_align_auto(radius=16, rate=1.0, state=None):
    """stm_set_align_auto: mode 2's parameters -- the search radius in rows (1 .. 32), the rate at which the field follows a
    frame's fit, and `state`: a float32 tensor of four elements on the GPU, {valid, a, b, c}, which carries the history from frame
    to frame (zero `valid` to reset it) -- the caller keeps it alive while the setting is in use; None = every frame on its own.
    Raises ValueError where the library refuses."""
    if state is not None:
        assert state.is_cuda and state.dtype == torch.float32 and state.is_contiguous() and state.numel() == 4
    if int(lib().stm_set_align_auto(int(radius), float(rate), _p(state) if state is not None else None)) != 0:
        raise ValueError("stm_set_align_auto(%d, %g) refused: %s" % (radius, rate, lib().stm_last_error().decode()))


def get_align():
    """stm_get_align: the calling thread's (mode, a, b, c, radius, rate) as the library holds it"""
    m = (C.c_int * 2)()
    v = (C.c_float * 4)()
    lib().stm_get_align(m, C.cast(v, f32p))
    return int(m[0]), float(v[0]), float(v[1]), float(v[2]), int(m[1]), float(v[3])


def d_align_rows(out, img, a, b, c):
    """stm_d_align_rows: img (uint8 [H][W][E] on the GPU) sampled at row y + a + b u + c v into out, which must not overlap img;
    only bytes 0 .. 2 of a pixel are written."""
    H, W, E = img.shape
    for t in (out, img):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    _use_current_stream()
    lib().stm_d_align_rows(_p(out), _p(img), H, W, E, float(a), float(b), float(c))


def d_rectify(out, img, rec, border=0):
    """stm_d_rectify: img (uint8 [H][W][E] on the GPU) through the rectification record rec (18 floats, host memory) into out, which
    must not overlap img; border 0 = taps outside are 0, 1 = clamped.  Only bytes 0 .. 2 of a pixel are written."""
    import numpy as np
    H, W, E = img.shape
    for t in (out, img):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    r = np.ascontiguousarray(rec, dtype=np.float32)
    assert r.shape == (18,)
    _use_current_stream()
    lib().stm_d_rectify(_p(out), _p(img), r.ctypes.data_as(f32p), H, W, E, int(border))


def d_align_fit(img_l, img_r, radius, rate, state, valid_blocks=None, profiles=None, sad=None):
    """stm_d_align_fit: the measurement of the automatic alignment as a stage -- the two unpacked images (uint8 [H][W][E] on the
    GPU) into the band profiles, their gradients' SADs, the fit, the update of `state` (float32, four elements on the GPU) in
    place; nothing synchronised.  valid_blocks (int32, 1), profiles (int32 [2][8][H]) and sad (int32 [8][4][2 radius + 1]) receive
    the intermediate results where given."""
    H, W, E = img_l.shape
    for t in (img_l, img_r):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    assert state.is_cuda and state.dtype == torch.float32 and state.is_contiguous() and state.numel() == 4
    for t, n in ((valid_blocks, 1), (profiles, 2 * 8 * H), (sad, 8 * 4 * (2 * int(radius) + 1))):
        assert t is None or (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n)
    _use_current_stream()
    lib().stm_d_align_fit(_p(img_l), _p(img_r), H, W, E, int(radius), float(rate), _p(state),
                          _p(valid_blocks) if valid_blocks is not None else None, _p(profiles) if profiles is not None else None,
                          _p(sad) if sad is not None else None)


def _lut768(lut):
    """a (3, 256) or (768,) table of bytes as a ctypes array the library copies from"""
    import numpy as np
    a = np.ascontiguousarray(lut)
    if a.dtype != np.uint8 or a.size != 768:
        raise ValueError("a balance table is 768 bytes of uint8 (B, G, R, 256 each), got %s %s" % (a.dtype, a.shape))
    return (C.c_uint8 * 768).from_buffer_copy(a.tobytes())


def set_balance(mode, lut=None):
    """stm_set_balance: the calling thread's colour balance between the eyes, applied to every frame call's input ahead of the
    matcher (after the alignment).  mode 0 = off (the default), 1 = given: the right eye through lut, a uint8 array of (3, 256)
    (B, G, R), 2 = measured: the tables fitted on every frame on the GPU with set_balance_auto's parameters.  Raises ValueError
    where the library refuses."""
    buf = _lut768(lut) if lut is not None else None
    if int(lib().stm_set_balance(int(mode), buf)) != 0:
        raise ValueError("stm_set_balance(%d) refused: %s" % (mode, lib().stm_last_error().decode()))


def set_balance_auto(max_shift=48, rate=1.0, state=None):
    """stm_set_balance_auto: mode 2's parameters -- the most levels a table moves a level by (0 .. 255), the rate at which the
    tables follow a frame's fit, and `state`: an int32 tensor of 769 elements on the GPU, {valid, 768 levels in 1/256}, which
    carries the history from frame to frame (zero `valid` to reset it) -- the caller keeps it alive while the setting is in use;
    None = every frame on its own.  Raises ValueError where the library refuses."""
    if state is not None:
        assert state.is_cuda and state.dtype == torch.int32 and state.is_contiguous() and state.numel() == 769
    if int(lib().stm_set_balance_auto(int(max_shift), float(rate), _p(state) if state is not None else None)) != 0:
        raise ValueError("stm_set_balance_auto(%d, %g) refused: %s" % (max_shift, rate, lib().stm_last_error().decode()))


def get_balance():
    """stm_get_balance: the calling thread's (mode, max_shift, rate, lut) as the library holds it; lut a (3, 256) uint8 array"""
    import numpy as np
    m = (C.c_int * 2)()
    r = C.c_float()
    t = (C.c_uint8 * 768)()
    lib().stm_get_balance(m, C.byref(r), t)
    return int(m[0]), int(m[1]), float(r.value), np.frombuffer(bytes(t), np.uint8).reshape(3, 256).copy()


def d_balance_fit(img_l, img_r, max_shift, rate, state, hist=None):
    """stm_d_balance_fit: the measurement of the colour balance as a stage -- the two unpacked images (uint8 [H][W][E] on the GPU)
    into six histograms, the fit, the update of `state` (int32, 769 elements on the GPU) in place; nothing synchronised.  hist
    (int32 [2][3][256]) receives the histograms where given."""
    H, W, E = img_l.shape
    for t in (img_l, img_r):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    assert state.is_cuda and state.dtype == torch.int32 and state.is_contiguous() and state.numel() == 769
    assert hist is None or (hist.is_cuda and hist.dtype == torch.int32 and hist.is_contiguous() and hist.numel() == 1536)
    _use_current_stream()
    lib().stm_d_balance_fit(_p(img_l), _p(img_r), H, W, E, int(max_shift), float(rate), _p(state), _p(hist) if hist is not None else None)


def d_balance_apply(out, img, lut=None, state=None):
    """stm_d_balance_apply: img (uint8 [H][W][E] on the GPU) through the three tables into out, which must not overlap img; only
    bytes 0 .. 2 of a pixel are written.  The tables are lut (a uint8 array of (3, 256) in host memory) or those of state (int32, 769
    elements on the GPU): exactly one of the two."""
    H, W, E = img.shape
    for t in (out, img):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    assert state is None or (state.is_cuda and state.dtype == torch.int32 and state.is_contiguous() and state.numel() == 769)
    _use_current_stream()
    lib().stm_d_balance_apply(_p(out), _p(img), H, W, E, _lut768(lut) if lut is not None else None, _p(state) if state is not None else None)


def set_cut(mode, thresh_permille=370, min_gap=1, state=None):
    """stm_set_cut: the calling thread's shot-change detector.  mode 0 = off (the default; the other arguments are ignored), 1 = on:
    every frame call first takes the left eye's signature and, on a cut, zeroes the `valid` word of the depth, alignment and balance
    states of mode 2 before their fits run.  `state`: an int32 tensor of 260 elements on the GPU, {valid, cut, since, score, sig[256]},
    zeroed at the start -- the caller keeps it alive while the setting is in use and reads the flag from state[1].  Raises
    ValueError where the library refuses (mode 1 without a state among the reasons)."""
    if state is not None:
        assert state.is_cuda and state.dtype == torch.int32 and state.is_contiguous() and state.numel() == 260
    if int(lib().stm_set_cut(int(mode), int(thresh_permille), int(min_gap), _p(state) if state is not None else None)) != 0:
        raise ValueError("stm_set_cut(%d, %d, %d) refused: %s" % (mode, thresh_permille, min_gap, lib().stm_last_error().decode()))


def get_cut():
    """stm_get_cut: the calling thread's (mode, thresh_permille, min_gap) as the library holds it"""
    out = (C.c_int * 3)()
    lib().stm_get_cut(out)
    return int(out[0]), int(out[1]), int(out[2])


def d_cut_detect(img_l, thresh_permille, min_gap, state, resets=(), sig=None):
    """stm_d_cut_detect: the shot-change detector as a stage -- the left image (uint8 [H][W][E] on the GPU) into its signature, the
    decision against `state` (int32, 260 elements on the GPU), updated in place; nothing synchronised.  resets: up to three tensors
    on the GPU (or None) whose first 32-bit word is zeroed on a cut; sig (int32, 256 elements) receives the signature where given."""
    H, W, E = img_l.shape
    assert img_l.is_cuda and img_l.dtype == torch.uint8 and img_l.is_contiguous()
    assert state.is_cuda and state.dtype == torch.int32 and state.is_contiguous() and state.numel() == 260
    assert sig is None or (sig.is_cuda and sig.dtype == torch.int32 and sig.is_contiguous() and sig.numel() == 256)
    resets = list(resets) + [None] * (3 - len(resets))
    assert len(resets) == 3
    for t in resets:
        assert t is None or (t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() >= 4)
    _use_current_stream()
    lib().stm_d_cut_detect(_p(img_l), H, W, E, int(thresh_permille), int(min_gap), _p(state), *[_p(t) if t is not None else None for t in resets],
                           _p(sig) if sig is not None else None)


ACTIVE_AUTO_DEFAULTS = (24, 10, 300, 12)  # thresh_luma, lit_permille, max_bar_permille, hold


def _rect4(rect):
    r = (C.c_int * 4)(*[int(v) for v in rect])
    return r


def _is_rect(t):
    return t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= 4


def set_active(mode, rect=None, fill=False, fill_disp=0.0):
    """stm_set_active: the calling thread's active picture area.  mode 0 = off (the default; the other arguments are ignored), 1 = the
    given rect = (top, bottom, left, right) -- rows [top, bottom), columns [left, right) of one eye --, 2 = measured on each frame's
    left eye on the GPU with set_active_auto's parameters.  With a mode on, depth mode 2 and the automatic overlay placement of every
    frame call are fitted under the rectangle, and with `fill` the maps the call hands back hold fill_disp outside it.  Raises
    ValueError where the library refuses."""
    if int(lib().stm_set_active(int(mode), _rect4(rect) if rect is not None else None, int(fill), float(fill_disp))) != 0:
        raise ValueError("stm_set_active(%d, %r, %r, %g) refused: %s" % (mode, rect, fill, fill_disp, lib().stm_last_error().decode()))


def set_active_auto(thresh_luma=24, lit_permille=10, max_bar_permille=300, hold=12, state=None):
    """stm_set_active_auto: mode 2's parameters (d_active_detect has their meaning), kept when the mode changes.  `state`: an int32
    tensor of 16 elements on the GPU, {valid, top, bottom, left, right, changed, H, W, cand[4], run[4]}, zeroed at the start -- the
    caller keeps it alive while the setting is in use; None = every frame measured on its own.  Raises ValueError where the library
    refuses."""
    if state is not None:
        assert state.is_cuda and state.dtype == torch.int32 and state.is_contiguous() and state.numel() == 16
    if int(lib().stm_set_active_auto(int(thresh_luma), int(lit_permille), int(max_bar_permille), int(hold),
                                     _p(state) if state is not None else None)) != 0:
        raise ValueError("stm_set_active_auto(%d, %d, %d, %d) refused: %s"
                         % (thresh_luma, lit_permille, max_bar_permille, hold, lib().stm_last_error().decode()))


def get_active():
    """stm_get_active: the calling thread's (mode, (top, bottom, left, right), fill, fill_disp, thresh_luma, lit_permille,
    max_bar_permille, hold) as the library holds it"""
    out = (C.c_int * 10)()
    fd = C.c_float(0.0)
    lib().stm_get_active(out, C.cast(C.byref(fd), f32p))
    return (int(out[0]), tuple(int(v) for v in out[1:5]), int(out[5]), float(fd.value), int(out[6]), int(out[7]), int(out[8]), int(out[9]))


def d_active_detect(img_l, state, thresh_luma=24, lit_permille=10, max_bar_permille=300, hold=12, restart=False, cut_state=None, counts=None):
    """stm_d_active_detect: the active picture area as a stage -- the lit pixels (luma above thresh_luma) of the left image (uint8
    [H][W][E] on the GPU) per row and column, the bars of this frame, and the update of `state` (int32, 16 elements on the GPU) under
    the hold rule, in place; nothing synchronised.  cut_state: stm_cut_detect's 260 ints on the GPU or None; counts (int32, H + W
    elements, rows first) receives the counts where given.  The rectangle is state[1:5]."""
    H, W, E = img_l.shape
    assert img_l.is_cuda and img_l.dtype == torch.uint8 and img_l.is_contiguous()
    assert state.is_cuda and state.dtype == torch.int32 and state.is_contiguous() and state.numel() == 16
    assert counts is None or (counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == H + W)
    if cut_state is not None:
        assert cut_state.is_cuda and cut_state.dtype == torch.int32 and cut_state.is_contiguous() and cut_state.numel() >= 2
    _use_current_stream()
    lib().stm_d_active_detect(_p(img_l), H, W, E, int(thresh_luma), int(lit_permille), int(max_bar_permille), int(hold), int(bool(restart)),
                              _p(state), _p(cut_state) if cut_state is not None else None, _p(counts) if counts is not None else None)


def d_active_fill(disp, rect, value):
    """stm_d_active_fill: every pixel of disp (float32 [H][W] on the GPU) outside rect (int32, four elements on the GPU: top, bottom,
    left, right; None = the whole map) becomes `value`, in place; the inside is not touched.  Nothing synchronised."""
    H, W = disp.shape
    assert disp.is_cuda and disp.dtype == torch.float32 and disp.is_contiguous()
    assert rect is None or _is_rect(rect)
    _use_current_stream()
    lib().stm_d_active_fill(_p(disp), H, W, _p(rect) if rect is not None else None, float(value))


def d_depth_fit_rect(disp_l, disp_r, disp_lo, disp_hi, max_gain, clip_permille, rate, state, rect):
    """stm_d_depth_fit_rect: d_depth_fit over the pixels inside rect only (int32, four elements on the GPU; None = d_depth_fit)."""
    H, W = disp_l.shape
    for t in (disp_l, disp_r):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (H, W)
    assert state.is_cuda and state.dtype == torch.float32 and state.is_contiguous() and state.numel() == 4
    assert rect is None or _is_rect(rect)
    _use_current_stream()
    lib().stm_d_depth_fit_rect(_p(disp_l), _p(disp_r), H, W, float(disp_lo), float(disp_hi), float(max_gain), int(clip_permille), float(rate),
                               _p(state), _p(rect) if rect is not None else None)


def d_overlay_fit_rect(disp_l, disp_r, overlay, x0, y0, view_rows, view_cols, limit_lo, limit_hi, state, rect, gain=1.0, conv=0.0,
                       near_permille=20, margin=1.0, pad=8, rate_near=1.0, rate_far=0.1, restart=False, cut_state=None):
    """stm_d_overlay_fit_rect: d_overlay_fit with the footprint's map rectangle moved into rect (int32, four elements on the GPU;
    None = d_overlay_fit): their intersection, or the picture lines nearest to a footprint that lies wholly in a bar."""
    H, W = disp_l.shape
    for t in (disp_l, disp_r):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (H, W)
    _check_overlay(overlay)
    assert state.is_cuda and state.dtype == torch.float32 and state.is_contiguous() and state.numel() == 4
    assert rect is None or _is_rect(rect)
    if cut_state is not None:
        assert cut_state.is_cuda and cut_state.dtype == torch.int32 and cut_state.is_contiguous() and cut_state.numel() >= 2
    _use_current_stream()
    lib().stm_d_overlay_fit_rect(_p(disp_l), _p(disp_r), H, W, _p(overlay), overlay.shape[0], overlay.shape[1], int(x0), int(y0), int(view_rows),
                                 int(view_cols), float(gain), float(conv), int(near_permille), float(margin), int(pad), float(limit_lo),
                                 float(limit_hi), float(rate_near), float(rate_far), int(bool(restart)), _p(state),
                                 _p(cut_state) if cut_state is not None else None, _p(rect) if rect is not None else None)


def d_view_prefilter(out, img, disp, num_views, strength=1.0, max_radius=8, gate=1.0, gain=1.0, conv=0.0):
    """stm_d_view_prefilter: img (uint8 [H][W][E] on the GPU) filtered by its own map disp (float32 [H][W]) into out, which must not
    overlap img; only bytes 0 .. 2 of a pixel are written.  gain, conv: the depth budget the views are rendered with (set_depth)."""
    H, W, E = img.shape
    for t in (out, img):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    assert disp.is_cuda and disp.dtype == torch.float32 and disp.is_contiguous() and disp.shape == (H, W)
    _use_current_stream()
    lib().stm_d_view_prefilter(_p(out), _p(img), _p(disp), H, W, E, int(num_views), float(strength), int(max_radius), float(gate),
                               float(gain), float(conv))


def d_mux_multiview_lens(views, out, mode, pitch, slope, centre):
    """stm_d_mux_multiview_lens: the views (a list of N uint8 [H][W][E] tensors on the GPU, views[0] = the right image ...
    views[N - 1] = the left image) interlaced into out (uint8 [Ho][Wo][E], only the first three bytes of a pixel are written)
    through the lens geometry; mode 1 or 2."""
    H, W, E = views[0].shape
    for t in views:
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.shape[2] == E
    tab = torch.tensor([t.data_ptr() for t in views], dtype=torch.int64).to(out.device)
    _use_current_stream()
    lib().stm_d_mux_multiview_lens(_p(tab), _p(out), len(views), int(mode), float(pitch), float(slope), float(centre), H, W,
                                   out.shape[0], out.shape[1], E)
    torch.cuda.current_stream().synchronize()  # the kernel reads the pointer table: keep it alive until it has run


def d_quilt_multiview(views, out, tiles_x, tiles_y, order=0, filter=0):
    """stm_d_quilt_multiview: the views (a list of N = tiles_x * tiles_y uint8 [H][W][E] tensors on the GPU, views[0] = the right
    image ... views[N - 1] = the left image) tiled into out (uint8 [Ho][Wo][E], only the first three bytes of a pixel are
    written); set_layout's order and filter."""
    H, W, E = views[0].shape
    for t in views:
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.shape[2] == E
    tab = torch.tensor([t.data_ptr() for t in views], dtype=torch.int64).to(out.device)
    _use_current_stream()
    lib().stm_d_quilt_multiview(_p(tab), _p(out), len(views), int(tiles_x), int(tiles_y), int(order), int(filter), H, W,
                                out.shape[0], out.shape[1], E)
    torch.cuda.current_stream().synchronize()  # the kernel reads the pointer table: keep it alive until it has run


def d_adcensus_stm(sbs, disp_l, disp_r, interlaced, p, stages=3):
    """stm_d_adcensus_stm: sbs uint8 [H][2W][3] on the GPU; outputs are written in place.
    stages: 1 = cost+aggregation+WTA, 2 = + refinement, 3 = full frame (views + interlacing); OR-ing 0x100 adds the
    scanline optimisation, OR-ing STAGE_SUBPIXEL the sub-pixel enhancement, OR-ing STAGE_INTERP the outlier interpolation,
    OR-ing STAGE_LINEAR_WARP (stage 3) the linear sampling of the views' warps."""
    assert sbs.is_cuda and sbs.dtype == torch.uint8 and sbs.is_contiguous()
    H, Wsbs, E = sbs.shape
    H, W = _eye_shape(H, Wsbs, disp_l)
    assert disp_l.shape == (H, W) and disp_r.shape == (H, W) and disp_l.dtype == torch.float32
    Ho, Wo = _out_size(interlaced, p)
    _use_current_stream()
    lib().stm_d_adcensus_stm(_p(sbs), _p(disp_l), _p(disp_r), _p(interlaced), H, Wsbs, W, Ho, Wo, E,
                             p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff,
                             p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, stages)


def d_adcensus_stm_t(sbs, disp_l, disp_r, interlaced, p, stages=3, prev_sbs=None, prev_disp_l=None, prev_disp_r=None,
                     alpha=TEMPORAL_DEFAULTS[0], thresh_color=TEMPORAL_DEFAULTS[1], thresh_disp=TEMPORAL_DEFAULTS[2]):
    """stm_d_adcensus_stm_t: d_adcensus_stm with the history of the temporal stabilisation.  With STAGE_TEMPORAL in `stages` and
    the previous frame's side-by-side input and output maps given, disp_l / disp_r are stabilised in place before the views are
    rendered; with all three None (the first frame) the call is d_adcensus_stm without the bit."""
    assert sbs.is_cuda and sbs.dtype == torch.uint8 and sbs.is_contiguous()
    H, Wsbs, E = sbs.shape
    H, W = _eye_shape(H, Wsbs, disp_l)
    assert disp_l.shape == (H, W) and disp_r.shape == (H, W) and disp_l.dtype == torch.float32
    if prev_sbs is not None:
        assert prev_sbs.is_cuda and prev_sbs.dtype == torch.uint8 and prev_sbs.is_contiguous() and prev_sbs.shape == sbs.shape
    for t in (prev_disp_l, prev_disp_r):
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (H, W)
    Ho, Wo = _out_size(interlaced, p)
    _use_current_stream()
    lib().stm_d_adcensus_stm_t(_p(sbs), _p(disp_l), _p(disp_r), _p(interlaced), H, Wsbs, W, Ho, Wo, E,
                               p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff,
                               p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, stages,
                               None if prev_sbs is None else _p(prev_sbs), None if prev_disp_l is None else _p(prev_disp_l),
                               None if prev_disp_r is None else _p(prev_disp_r), float(alpha), int(thresh_color), float(thresh_disp))


def _nv12_planes(y, uv, num_cols_sbs):
    """(H, Wsbs, pitch_y, pitch_uv) of a pair of 2-D uint8 plane tensors whose rows may be pitched (stride(0) >= the row, stride(1) == 1)"""
    for t in (y, uv):
        assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1)
    H = y.shape[0]
    Wsbs = y.shape[1] if num_cols_sbs is None else num_cols_sbs
    assert uv.shape[0] * 2 == H and y.shape[1] >= Wsbs and uv.shape[1] >= 2 * ((Wsbs + 1) // 2)
    return H, Wsbs, y.stride(0), uv.stride(0)


def d_demux_nv12(img_l, img_r, y, uv, matrix=0, num_cols_sbs=None):
    """stm_d_demux_nv12: the two views of a side-by-side NV12 frame converted to BGR into img_l / img_r (uint8 [H][W][E], only the
    first three bytes of a pixel are written).  y uint8 [H][>= Wsbs] and uv uint8 [H / 2][>= Wsbs] are 2-D tensors whose row
    stride is the plane's pitch (a view into a larger allocation is fine); matrix: 0 / 1 = BT.601 / BT.709 limited range, 2 / 3 =
    BT.601 / BT.709 full range."""
    H, Wsbs, pitch_y, pitch_uv = _nv12_planes(y, uv, num_cols_sbs)
    W, E = img_l.shape[1], img_l.shape[2]
    for t in (img_l, img_r):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    _use_current_stream()
    lib().stm_d_demux_nv12(_p(img_l), _p(img_r), _p(y), pitch_y, _p(uv), pitch_uv, H, Wsbs, W, E, int(matrix))


def d_adcensus_stm_nv12(y, uv, disp_l, disp_r, interlaced, p, stages=3, matrix=0, img_l=None, img_r=None, prev_img_l=None, prev_img_r=None,
                        prev_disp_l=None, prev_disp_r=None, alpha=TEMPORAL_DEFAULTS[0], thresh_color=TEMPORAL_DEFAULTS[1],
                        thresh_disp=TEMPORAL_DEFAULTS[2], num_cols_sbs=None, elem_sz=3):
    """stm_d_adcensus_stm_nv12: d_adcensus_stm_t on a side-by-side NV12 frame (planes as for d_demux_nv12), the conversion fused
    into the frame's first kernel.  img_l / img_r (uint8 [H][W][E], optional, required with STAGE_TEMPORAL) receive the converted
    split images: they are the next frame's prev_img_l / prev_img_r.  elem_sz is taken from img_l where that is given."""
    H, Wsbs, pitch_y, pitch_uv = _nv12_planes(y, uv, num_cols_sbs)
    W = disp_l.shape[1]
    if get_packing() != PACKING_OFF:  # the planes hold the packed frame: the unpacked eye's size is disp_l's
        H = _eye_shape(H, Wsbs, disp_l)[0]
    assert disp_l.shape == (H, W) and disp_r.shape == (H, W) and disp_l.dtype == torch.float32
    E = elem_sz if img_l is None else img_l.shape[2]
    for t in (img_l, img_r, prev_img_l, prev_img_r):
        if t is not None:
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    for t in (prev_disp_l, prev_disp_r):
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (H, W)
    Ho, Wo = _out_size(interlaced, p)

    def opt(t):
        return None if t is None else _p(t)
    _use_current_stream()
    lib().stm_d_adcensus_stm_nv12(_p(y), pitch_y, _p(uv), pitch_uv, int(matrix), _p(disp_l), _p(disp_r), _p(interlaced), H, Wsbs, W, Ho, Wo, E,
                                  p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                                  p.thresh_s, p.thresh_h, stages, opt(prev_img_l), opt(prev_img_r), opt(prev_disp_l), opt(prev_disp_r),
                                  float(alpha), int(thresh_color), float(thresh_disp), opt(img_l), opt(img_r))


def d_adcensus_stm_2s(sbs, disp_l, disp_r, interlaced, p, disp_rows, disp_cols, disp_scale, stages=3):
    """stm_d_adcensus_stm_2s: the reduced-resolution frame (match at disp_rows x disp_cols, maps scaled up by 1 / disp_scale,
    views rendered at full size) with a `stages` word: 3, optionally OR-ed with 0x100, STAGE_SUBPIXEL, STAGE_INTERP (on the
    reduced pair), STAGE_LINEAR_WARP (the render) and STAGE_GUIDED_UP (the up-scale).  stages = 3 is stm_d_adcensus_stm_2."""
    assert sbs.is_cuda and sbs.dtype == torch.uint8 and sbs.is_contiguous()
    H, Wsbs, E = sbs.shape
    W = Wsbs // 2
    assert disp_l.shape == (H, W) and disp_r.shape == (H, W) and disp_l.dtype == torch.float32
    Ho, Wo = _out_size(interlaced, p)
    _use_current_stream()
    lib().stm_d_adcensus_stm_2s(_p(sbs), _p(disp_l), _p(disp_r), _p(interlaced), H, Wsbs, W, Ho, Wo, disp_rows, disp_cols, E,
                                disp_scale, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff,
                                p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, stages)


def d_adcensus_stm_2t(sbs, disp_l, disp_r, interlaced, p, disp_rows, disp_cols, disp_scale, stages=3, prev_sbs=None, prev_disp_l=None,
                      prev_disp_r=None, alpha=TEMPORAL_DEFAULTS[0], thresh_color=TEMPORAL_DEFAULTS[1], thresh_disp=TEMPORAL_DEFAULTS[2]):
    """stm_d_adcensus_stm_2t: d_adcensus_stm_2s with the history of the temporal stabilisation.  With STAGE_TEMPORAL in `stages` and
    the previous frame's side-by-side input and full-size output maps given, the up-scaled disp_l / disp_r are stabilised in place
    before the views are rendered; with all three None (the first frame) the call is d_adcensus_stm_2s without the bit."""
    assert sbs.is_cuda and sbs.dtype == torch.uint8 and sbs.is_contiguous()
    H, Wsbs, E = sbs.shape
    W = Wsbs // 2
    assert disp_l.shape == (H, W) and disp_r.shape == (H, W) and disp_l.dtype == torch.float32
    if prev_sbs is not None:
        assert prev_sbs.is_cuda and prev_sbs.dtype == torch.uint8 and prev_sbs.is_contiguous() and prev_sbs.shape == sbs.shape
    for t in (prev_disp_l, prev_disp_r):
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (H, W)
    Ho, Wo = _out_size(interlaced, p)

    def opt(t):
        return None if t is None else _p(t)
    _use_current_stream()
    lib().stm_d_adcensus_stm_2t(_p(sbs), _p(disp_l), _p(disp_r), _p(interlaced), H, Wsbs, W, Ho, Wo, disp_rows, disp_cols, E,
                                disp_scale, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff,
                                p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, stages, opt(prev_sbs), opt(prev_disp_l), opt(prev_disp_r),
                                float(alpha), int(thresh_color), float(thresh_disp))


def d_adcensus_stm_2nv12(y, uv, disp_l, disp_r, interlaced, p, disp_rows, disp_cols, disp_scale, stages=3, matrix=0, img_l=None, img_r=None,
                         prev_img_l=None, prev_img_r=None, prev_disp_l=None, prev_disp_r=None, alpha=TEMPORAL_DEFAULTS[0],
                         thresh_color=TEMPORAL_DEFAULTS[1], thresh_disp=TEMPORAL_DEFAULTS[2], num_cols_sbs=None, elem_sz=3):
    """stm_d_adcensus_stm_2nv12: d_adcensus_stm_2t on a side-by-side NV12 frame (planes as for d_demux_nv12), the conversion fused
    into the frame's first kernel.  img_l / img_r (uint8 [H][W][E], optional, required with STAGE_TEMPORAL) receive the converted
    split images: they are the next frame's prev_img_l / prev_img_r.  elem_sz is taken from img_l where that is given."""
    H, Wsbs, pitch_y, pitch_uv = _nv12_planes(y, uv, num_cols_sbs)
    W = disp_l.shape[1]
    assert disp_l.shape == (H, W) and disp_r.shape == (H, W) and disp_l.dtype == torch.float32
    E = elem_sz if img_l is None else img_l.shape[2]
    for t in (img_l, img_r, prev_img_l, prev_img_r):
        if t is not None:
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    for t in (prev_disp_l, prev_disp_r):
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (H, W)
    Ho, Wo = _out_size(interlaced, p)

    def opt(t):
        return None if t is None else _p(t)
    _use_current_stream()
    lib().stm_d_adcensus_stm_2nv12(_p(y), pitch_y, _p(uv), pitch_uv, int(matrix), _p(disp_l), _p(disp_r), _p(interlaced), H, Wsbs, W, Ho, Wo,
                                   disp_rows, disp_cols, E, disp_scale, p.num_views, p.angle, p.num_disp, p.zero_disp, p.ad_coeff,
                                   p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd, p.thresh_s, p.thresh_h, stages, opt(prev_img_l), opt(prev_img_r),
                                   opt(prev_disp_l), opt(prev_disp_r), float(alpha), int(thresh_color), float(thresh_disp), opt(img_l),
                                   opt(img_r))


def _low_outputs(img_l, img_r, low_l, low_r, census_l, census_r):
    H, W, E = img_l.shape
    h, w = low_l.shape[:2]
    for t, shape in ((img_l, (H, W, E)), (img_r, (H, W, E)), (low_l, (h, w, E)), (low_r, (h, w, E))):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == shape
    for t in (census_l, census_r):
        if t is not None:  # 32-bit words: int32 tensors (torch has no arithmetic on uint32), viewed as uint32 by the caller
            assert t.is_cuda and t.element_size() == 4 and t.is_contiguous() and t.shape == (h, w)
    return H, W, E, h, w


def d_demux_sbs_low(img_l, img_r, low_l, low_r, sbs, census_l=None, census_r=None, num_cols_sbs=None):
    """stm_d_demux_sbs_low: the reduced-resolution frame's front as a stage.  From sbs (uint8 [H][Wsbs][E] on the GPU): the split
    images img_l / img_r (uint8 [H][W][E]), the bilinearly reduced images low_l / low_r (uint8 [h][w][E]) and, where given, the
    reduced images' 32-bit census words census_l / census_r (4-byte integer tensors [h][w]).  Only the first three bytes of a pixel
    are written."""
    H, W, E, h, w = _low_outputs(img_l, img_r, low_l, low_r, census_l, census_r)
    assert sbs.is_cuda and sbs.dtype == torch.uint8 and sbs.is_contiguous() and sbs.shape[0] == H and sbs.shape[2] == E
    Wsbs = sbs.shape[1] if num_cols_sbs is None else num_cols_sbs
    assert Wsbs == sbs.shape[1]
    _use_current_stream()
    lib().stm_d_demux_sbs_low(_p(img_l), _p(img_r), _p(low_l), _p(low_r), None if census_l is None else _p(census_l),
                              None if census_r is None else _p(census_r), _p(sbs), H, Wsbs, W, h, w, E)


def d_demux_nv12_low(img_l, img_r, low_l, low_r, y, uv, matrix=0, census_l=None, census_r=None, num_cols_sbs=None):
    """stm_d_demux_nv12_low: d_demux_sbs_low on a side-by-side NV12 frame (planes as for d_demux_nv12): the reduced images are the
    reduction of the converted split images."""
    H, W, E, h, w = _low_outputs(img_l, img_r, low_l, low_r, census_l, census_r)
    Hy, Wsbs, pitch_y, pitch_uv = _nv12_planes(y, uv, num_cols_sbs)
    assert Hy == H
    _use_current_stream()
    lib().stm_d_demux_nv12_low(_p(img_l), _p(img_r), _p(low_l), _p(low_r), None if census_l is None else _p(census_l),
                               None if census_r is None else _p(census_r), _p(y), pitch_y, _p(uv), pitch_uv, H, Wsbs, W, h, w, E, int(matrix))


def plane_table(slab):
    """Device table of plane pointers for a contiguous [D][H][W] float tensor."""
    D = slab.shape[0]
    stride = slab.stride(0) * slab.element_size()
    ptrs = torch.tensor([slab.data_ptr() + d * stride for d in range(D)], dtype=torch.int64)
    return ptrs.to(slab.device)


def d_ci_adcensus(img_l, img_r, slab, ad_coeff, census_coeff, num_disp, zero_disp):
    """stm_d_ci_adcensus: slab float32 [2][D][H][W]; returns (d_tab_l, d_tab_r) device pointer tables."""
    H, W, E = img_l.shape
    _use_current_stream()
    tab_l = torch.zeros(num_disp, dtype=torch.int64, device=slab.device)
    tab_r = torch.zeros(num_disp, dtype=torch.int64, device=slab.device)
    h_l = (f32p * num_disp)()
    h_r = (f32p * num_disp)()
    lib().stm_d_ci_adcensus(_p(img_l), _p(img_r), _p(tab_l), _p(tab_r), C.cast(h_l, f32pp), C.cast(h_r, f32pp),
                            _p(slab), ad_coeff, census_coeff, num_disp, zero_disp, H, W, E)
    torch.cuda.current_stream().synchronize()  # h_l/h_r are read by the async table upload
    return tab_l, tab_r


def d_ca_cross(img, cost_tab, scratch, cross, ucd, lcd, usd, lsd, num_disp):
    """stm_d_ca_cross: result lands in the planes cost_tab points at; cross uint8 [4][H][W] receives the arms."""
    H, W, E = img.shape
    _use_current_stream()
    acost_tab = torch.zeros(num_disp, dtype=torch.int64, device=img.device)
    h_a = (f32p * num_disp)()
    cross_tab = torch.tensor([cross[k].data_ptr() for k in range(4)], dtype=torch.int64).to(img.device)
    lib().stm_d_ca_cross(_p(img), _p(cost_tab), _p(acost_tab), C.cast(h_a, f32pp), _p(scratch), _p(cross_tab),
                         ucd, lcd, usd, lsd, num_disp, H, W, E)
    torch.cuda.current_stream().synchronize()
    return cross_tab


def d_dc_wta(cost_tab, disp, num_disp, zero_disp):
    H, W = disp.shape
    _use_current_stream()
    lib().stm_d_dc_wta(_p(cost_tab), _p(disp), num_disp, zero_disp, H, W)


def d_dc_hslo_view(cost_tab, disp, img_own, img_other, T, H1, H2, num_disp, zero_disp, view=0):
    """stm_d_dc_hslo_view: scanline optimisation + WTA of one view on the aggregated volume behind cost_tab; disp float32 [H][W]
    receives the map.  view 0 = the left view (stm_d_dc_hslo), 1 = the right view; img_own is the view's own image, img_other the
    other one, both uint8 [H][W][E] on the GPU."""
    H, W, E = img_own.shape
    assert img_other.shape == img_own.shape and tuple(disp.shape) == (H, W)
    for t in (img_own, img_other):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    assert disp.is_cuda and disp.dtype == torch.float32 and disp.is_contiguous()
    _use_current_stream()
    lib().stm_d_dc_hslo_view(_p(cost_tab), _p(disp), _p(img_own), _p(img_other), float(T), float(H1), float(H2), int(num_disp),
                             int(zero_disp), H, W, E, int(view))


def d_dc_subpixel(cost_tab, disp, num_disp, zero_disp):
    """stm_d_dc_subpixel: disp float32 [H][W] on the GPU refined in place on the aggregated volume behind cost_tab."""
    H, W = disp.shape
    _use_current_stream()
    lib().stm_d_dc_subpixel(_p(cost_tab), _p(disp), num_disp, zero_disp, H, W)


def d_dr_interp(disp, outliers, img):
    """stm_d_dr_interp: disp float32 [H][W] on the GPU refined in place where outliers (uint8 [H][W]) != 0; img uint8 [H][W][E]
    is the same view's image.  outliers and img are only read."""
    H, W = disp.shape
    assert disp.is_cuda and disp.dtype == torch.float32 and disp.is_contiguous()
    assert outliers.shape == (H, W) and outliers.dtype == torch.uint8 and outliers.is_contiguous()
    assert img.shape[:2] == (H, W) and img.dtype == torch.uint8 and img.is_contiguous()
    _use_current_stream()
    lib().stm_d_dr_interp(_p(disp), _p(outliers), _p(img), H, W, img.shape[2])


def d_dibr_dbm_lin(out, img_l, img_r, disp_l, disp_r, mask_l, mask_r, shift):
    """stm_d_dibr_dbm_lin: one synthesised view written to out (uint8 [H][W][E], cleared first when E > 3) from the two images,
    the two disparity maps and the two masks, both warps fetched at the fractional coordinate; mask blur gaussian(10, 15)."""
    H, W, E = img_l.shape
    for t in (out, img_l, img_r):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    for t in (disp_l, disp_r, mask_l, mask_r):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (H, W)
    _use_current_stream()
    lib().stm_d_dibr_dbm_lin(_p(out), _p(img_l), _p(img_r), _p(disp_l), _p(disp_r), None, None, _p(mask_l), _p(mask_r),
                             float(shift), H, W, E)


def d_disp_upsample(out, disp_low, img_low, img, up, sigma_color=15.0):
    """stm_d_disp_upsample: out float32 [H][W] on the GPU from the low-resolution map disp_low float32 [h][w], the image it was
    computed on (img_low uint8 [h][w][E]) and the guide image img uint8 [H][W][E]; the values are multiplied by `up`.  Only out
    is written."""
    H, W = out.shape
    h, w = disp_low.shape
    for t in (out, disp_low):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    E = img.shape[2]
    assert img.shape == (H, W, E) and img_low.shape == (h, w, E)
    for t in (img, img_low):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    _use_current_stream()
    lib().stm_d_disp_upsample(_p(out), _p(disp_low), _p(img_low), _p(img), H, W, h, w, E, float(up), float(sigma_color))


def d_disp_temporal(disp, disp_prev, img, img_prev, alpha=TEMPORAL_DEFAULTS[0], thresh_color=TEMPORAL_DEFAULTS[1],
                    thresh_disp=TEMPORAL_DEFAULTS[2]):
    """stm_d_disp_temporal: disp float32 [H][W] on the GPU stabilised in place against disp_prev, the map the previous frame put
    out, where the colour between img_prev and img (uint8 [H][W][E]) and the disparity stayed inside the gates.  Only disp is
    written."""
    H, W = disp.shape
    for t in (disp, disp_prev):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (H, W)
    E = img.shape[2]
    for t in (img, img_prev):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (H, W, E)
    _use_current_stream()
    lib().stm_d_disp_temporal(_p(disp), _p(disp_prev), _p(img), _p(img_prev), H, W, E, float(alpha), int(thresh_color), float(thresh_disp))


def prof_enable(on=True):
    """True / 1: HIP events around every named kernel; 2: around the aggregation kernels only; False / 0: off."""
    lib().stm_prof_enable(int(on))


def prof_reset():
    lib().stm_prof_reset()


def prof_read(name):
    ms = C.c_float(0.0)
    n = lib().stm_prof_read(name.encode(), C.byref(ms))
    return n, float(ms.value)
