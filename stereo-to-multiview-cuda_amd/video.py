"""Side-by-side frame sequences (SURVEY.md section 8f rows N1 + N4): the headless analogue of the reference's
video driver (video_io.cpp:42-224).  The OpenCV capture / window is replaced by an iterator of frames (a directory
of BMPs, a list of arrays, ...) and writers for what the viewer would show (interlaced frame, disparity maps
normalised like cv::normalize(..., 0, 1, CV_MINMAX), video_io.cpp:163-164)."""
import ctypes as C
import glob
import os

import numpy as np

from . import bmp_io
from ._lib import f32p, lib, u8p

# FrameStream(cut=...)'s and --cut's default (thresh_permille, min_gap).  370: DESIGN section 25 (the geometric mean of the largest
# non-cut and the smallest cut score on the committed images, rounded to 10).  3: a flash lasts one or two frames, so the frame that
# returns from it comes at most two frames after the flash's own cut and is suppressed; no edited shot is shorter than three frames.
CUT_DEFAULT = (370, 3)
# FrameStream(active_auto=True)'s and --active-auto's default (thresh_luma, lit_permille, max_bar_permille, hold): the C calls' own
# (DESIGN section 28).  24 clears limited-range black (16) plus codec noise; 12 frames is half a second of film.
ACTIVE_AUTO_DEFAULT = (24, 10, 300, 12)


class FrameStream:
    """Pipelined adcensus_stm over a sequence: submit() frames, collect() results in order (two in flight).
    input_format "bgr" (the default): a frame is a side-by-side BGR array uint8 [H][2W][3].  "nv12": a frame is uint8 [H * 3 / 2][2W],
    the Y plane followed by the interleaved UV plane, as a decoder or read_nv12_sequence delivers it; `matrix` selects the colour
    conversion (stm_demux_nv12: 0 / 1 = BT.601 / BT.709 limited range, 2 / 3 = full range).  lens = (mode, pitch, slope, centre): the
    panel's calibration (set_lens); None = the reference's interlacer.  depth = (gain, conv): the manual depth budget (set_depth mode 1);
    depth_auto = (disp_lo, disp_hi[, max_gain, clip_permille, rate]): the automatic one (mode 2), fitted to every frame on the GPU;
    at most one of the two.  packing = (packing, swap, filter, gap): the frames come packed (stm_set_packing's settings: half-width
    side by side, top and bottom, ...); num_rows x num_cols stay the size of an unpacked eye, and a frame is then [rows_f][Wsbs][3]
    (NV12: [rows_f * 3 / 2][Wsbs]) with Wsbs = 2 * (packed eye's columns) + gap for the side-by-side packings and num_cols for the
    top-and-bottom ones: the shape `in_shape` holds.  layout = (1, tiles_x, tiles_y, order, filter): the frames come out as a
    quilt of tiles_x x tiles_y whole views (set_layout); None = the interlaced frame.  match = (h, w, disp_scale): every frame is the
    reduced-resolution frame -- matched at h x w, the maps scaled up by 1 / disp_scale, the views rendered at full size -- and
    `stages` may then carry 0x1000 (the guided up-sampler); None = the full-resolution frame.  Not together with a packing.
    output = (1, matrix): the quilt comes out as NV12 (set_output), each frame uint8 [out_rows * 3 / 2][out_cols], the Y plane followed
    by the interleaved UV plane; None = BGR.  Needs a layout.  overlay = (max_rows, max_cols): the stream composites an overlay of up
    to that size into its frames (set_overlay; .overlay() sets the one in force); None = none.  Not together with an NV12 output.
    overlay_auto = (limit_lo, limit_hi[, near_permille, margin, pad, rate_near, rate_far]): the overlay's disparity is fitted on every
    frame on the GPU to the maps under the overlay (set_overlay_auto) and .overlay()'s own disparity is ignored; needs `overlay`;
    .overlay_depth() reads the state of the last collected frame.
    antialias = (strength, max_radius, gate): view antialiasing (set_antialias mode 1) -- both images filtered by their own maps
    before the views are rendered from them; None = off.  align = (a, b, c): the right eye of every frame sampled at row
    y + a + b u + c v ahead of the matcher (set_align mode 1); align_auto = (radius[, rate]): the field measured on every frame on
    the GPU (mode 2); at most one of the two; .align() reads the field of the last collected frame.  balance = a uint8 array of
    (3, 256): the right eye of every frame through these tables (B, G, R) ahead of the matcher, after the alignment (set_balance mode
    1); balance_auto = (max_shift[, rate]): the tables fitted on every frame on the GPU (mode 2); at most one of the two; .balance()
    reads the tables of the last collected frame.  cut = (thresh_permille, min_gap) or True (CUT_DEFAULT): the shot-change detector
    (set_cut mode 1) -- at a cut the depth_auto, align_auto and balance_auto states start afresh on the GPU; .cut() reads (cut, score,
    since) of the last collected frame.  active = (top, bottom, left, right): the picture's rectangle inside a letterboxed or
    pillarboxed frame (set_active mode 1); active_auto = (thresh_luma, lit_permille, max_bar_permille, hold) or True
    (ACTIVE_AUTO_DEFAULT): the rectangle measured on every frame on the GPU (mode 2), restarted at a cut; at most one of the two.
    depth_auto and overlay_auto are then fitted under the rectangle.  active_fill = a disparity: the maps that come back hold it in
    the bars; None = the maps as matched.  .active() reads (top, bottom, left, right, changed) of the last collected frame.
    maps = (format, which, lo, hi) or a format alone: what the two disparity maps of a frame come back as (set_maps) -- "f32" (the
    default: float32 arrays), "none" (collect() and collect_view() return None for both), "u8" or "u16": depth planes of one code per
    pixel, code 0 at map value lo and the largest code at hi (lo > hi: near = dark), of the maps `which` selects ("left", "right" or
    "both"; or 0, 1, 2) -- the other one comes back as None.  The float maps are computed either way; only the download changes.
    depth_input = (format, lo, hi[, fill, gate]): the frames are one image and its depth plane (set_depth_input) -- format "f32", "u8"
    or "u16", lo and hi the map values of code 0 and of the largest code (f32: the limits the values are clamped to), fill 0 =
    constant extension of the background into the holes, 1 = continue the background where the mirror pixel lies within `gate` of it.
    The image is the left eye, uint8 [H][depth_pitch][3] (depth_pitch = num_cols unless given), the plane [H][W] of disparities
    x_right - x_left (smaller is nearer); submit_depth(img, plane) takes the two, pack_depth_frame lays them out as submit() and
    input_buffer() see them.  The second eye is synthesised on the GPU and nothing is matched: collect() returns the decoded plane as
    disp_l and the synthesised right map as disp_r.  Not together with NV12 input, a packing, a match size, an alignment, a balance
    or stages beyond 3 | 0x800.
    rectify = (rec_l, rec_r[, border]): every frame's eyes are first remapped through their rectification records (set_rectify;
    stm_amd.rectify.record makes one from a camera calibration), ahead of every other setting: the stream is then, by definition,
    the stream without it on the rectified pairs.  border 0 (the default) = taps outside an eye are 0, 1 = clamped.  Not together
    with depth_input.
    depth_video = (format, matrix, packing, swap, filter, gap, range, dfilter, dgate, lo, hi[, fill, gate]): the frames are packed
    2D-plus-depth video frames (set_depth_video; include/stm_depth_video.h) -- format "bgr" or "nv12" with its conversion matrix; the
    image is eye 0 and its depth, a grey picture, eye 1 of the packing (the settings of `packing`; filter expands the image); range 0
    = codes 0 .. 255, 1 = limited-range video grey; dfilter 1 expands a squeezed depth picture linearly where neighbours lie within
    dgate codes, 0 replicates; lo and hi are the map values of the lowest and the highest code; fill and gate as depth_input's.
    submit() takes the packed frame as it is, `in_shape` as under packing= ([rows_f][Wsbs][3], NV12 [rows_f * 3 / 2][Wsbs]; depth_pitch
    = a row length larger than the packing needs).  Not together with depth_input, input_format "nv12", packing, match, an alignment, a
    balance, rectify or stages beyond 3 | 0x800."""

    def __init__(self, num_rows, num_cols, params, out_rows=None, out_cols=None, stages=3, input_format="bgr", matrix=0, lens=None,
                 depth=None, depth_auto=None, packing=None, layout=None, match=None, output=None, overlay=None,
                 antialias=None, align=None, align_auto=None, balance=None, balance_auto=None, cut=None, overlay_auto=None,
                 active=None, active_auto=None, active_fill=None, maps=None, depth_input=None, depth_pitch=None, rectify=None,
                 depth_video=None):
        self.H, self.W = num_rows, num_cols
        self._maps = (0, 2)
        self._depth_input = None
        self.packing = tuple(int(v) for v in packing) if packing is not None else (0, 0, 0, 0)
        self.Wsbs, self.rows_f = packed_frame_geometry(num_rows, num_cols, self.packing)
        if depth_input is not None and packing is None:  # one image a frame: its rows are num_cols pixels unless the caller says otherwise
            self.Wsbs = int(depth_pitch) if depth_pitch is not None else num_cols
        if depth_video is not None and packing is None and depth_input is None:  # one packed frame: the geometry of its own packing
            self.Wsbs = packed_frame_geometry(num_rows, num_cols, tuple(depth_video[2:6]))[0]
            if depth_pitch is not None:
                self.Wsbs = int(depth_pitch)
        self._nv12 = False
        self.in_shape = (self.rows_f, self.Wsbs, 3)
        self.Ho, self.Wo = out_rows or num_rows, out_cols or num_cols
        self.out_shape = (self.Ho, self.Wo, 3)
        p = params
        self._h = lib().stm_stream_create(num_rows, self.Wsbs, num_cols, self.Ho, self.Wo, 3, p.num_views, p.angle,
                                          p.num_disp, p.zero_disp, p.ad_coeff, p.census_coeff, p.ucd, p.lcd, p.usd, p.lsd,
                                          p.thresh_s, p.thresh_h)
        if match is not None:  # before the stages: 0x1000 needs it
            self.set_match_size(*match)
        if stages != 3:
            self.set_stages(stages)
        if packing is not None:
            self.set_packing(*self.packing)
        if input_format != "bgr":
            self.set_input(input_format, matrix)
        if depth_input is not None:
            self.set_depth_input(*depth_input)
        if depth_video is not None:
            self.set_depth_video(*depth_video)
        if rectify is not None:
            self.set_rectify(*rectify)
        if lens is not None:
            self.set_lens(*lens)
        if layout is not None:
            self.set_layout(*layout)
        if output is not None:
            self.set_output(*output)
        if depth is not None and depth_auto is not None:
            raise ValueError("FrameStream: depth and depth_auto are mutually exclusive")
        if depth is not None:
            self.set_depth(1, *depth)
        if depth_auto is not None:
            self.set_depth_auto(*depth_auto)
            self.set_depth(2)
        if overlay is not None:
            self.set_overlay(*overlay)
        if overlay_auto is not None:
            self.set_overlay_auto(1, *overlay_auto)
        if antialias is not None:
            self.set_antialias(1, *antialias)
        if align is not None and align_auto is not None:
            raise ValueError("FrameStream: align and align_auto are mutually exclusive")
        if align is not None:
            self.set_align(1, *align)
        if align_auto is not None:
            self.set_align_auto(*align_auto)
            self.set_align(2)
        if balance is not None and balance_auto is not None:
            raise ValueError("FrameStream: balance and balance_auto are mutually exclusive")
        if balance is not None:
            self.set_balance(1, balance)
        if balance_auto is not None:
            self.set_balance_auto(*balance_auto)
            self.set_balance(2)
        if cut is not None and cut is not False:
            self.set_cut(1, *(CUT_DEFAULT if cut is True else cut))
        if active is not None and active_auto is not None and active_auto is not False:
            raise ValueError("FrameStream: active and active_auto are mutually exclusive")
        fill = (0, 0.0) if active_fill is None else (1, float(active_fill))
        if active is not None:
            self.set_active(1, active, *fill)
        elif active_auto is not None and active_auto is not False:
            self.set_active(2, None, *fill, *(ACTIVE_AUTO_DEFAULT if active_auto is True else active_auto))
        elif active_fill is not None:
            raise ValueError("FrameStream: active_fill needs active or active_auto")
        if maps is not None:
            self.set_maps(*((maps,) if isinstance(maps, str) else maps))

    def set_depth_input(self, format, lo=0.0, hi=0.0, fill=0, gate=0.0):
        """stm_stream_input_depth: the frames are an image and its depth plane -- format "f32", "u8" or "u16" (or 0, 2, 3), None or
        "off" (or -1) = side-by-side frames again; lo, hi, fill and gate as FrameStream's depth_input.  Buffers handed out by
        input_buffer() before this call are void.  Only before the first submit.  Raises ValueError where the library refuses."""
        fmt = {"f32": 0, "u8": 2, "u16": 3, "off": -1, None: -1}.get(format, format)
        if not isinstance(fmt, int):
            raise ValueError("FrameStream.set_depth_input: format %r" % (format,))
        if int(lib().stm_stream_input_depth(self._h, fmt, float(lo), float(hi), int(fill), float(gate))) != 0:
            raise ValueError("stm_stream_input_depth(%r, %g, %g, %d, %g) refused: %s" % (format, lo, hi, fill, gate, lib().stm_last_error().decode()))
        self._depth_input = None if fmt < 0 else {0: np.dtype("<f4"), 2: np.dtype(np.uint8), 3: np.dtype("<u2")}[fmt]

    def set_depth_video(self, format, matrix=0, packing=0, swap=0, filter=0, gap=0, range=0, dfilter=0, dgate=0, lo=0.0, hi=0.0, fill=0,
                        gate=0.0):
        """stm_stream_input_packed_depth: the frames are packed 2D-plus-depth video frames -- format "bgr" or "nv12" (or 0, 1), None or
        "off" (or -1) = side-by-side frames again; the other arguments as FrameStream's depth_video.  `in_shape` follows the packing;
        buffers handed out by input_buffer() before this call are void.  Only before the first submit.  Raises ValueError where the
        library refuses."""
        fmt = {"bgr": 0, "nv12": 1, "off": -1, None: -1}.get(format, format)
        if not isinstance(fmt, int):
            raise ValueError("FrameStream.set_depth_video: format %r" % (format,))
        args = (fmt, int(matrix), int(packing), int(swap), int(filter), int(gap), int(range), int(dfilter), int(dgate), float(lo), float(hi),
                int(fill), float(gate))
        if int(lib().stm_stream_input_packed_depth(self._h, *args)) != 0:
            raise ValueError("stm_stream_input_packed_depth%r refused: %s" % (args, lib().stm_last_error().decode()))
        self.rows_f = self.H if fmt < 0 else packed_frame_geometry(self.H, self.W, args[2:6])[1]
        self._nv12 = fmt == 1
        self.in_shape = (self.rows_f * 3 // 2, self.Wsbs) if fmt == 1 else (self.rows_f, self.Wsbs, 3)

    def set_rectify(self, rec_l, rec_r=None, border=0):
        """stm_stream_rectify: both eyes of every frame through their records (18 floats each, stm_amd.rectify.record) before anything
        else is done with the frame; rec_l None = off.  Only before the first submit.  Raises ValueError where the library refuses."""
        if rec_l is None:
            if int(lib().stm_stream_rectify(self._h, 0, None, 0)) != 0:
                raise ValueError("stm_stream_rectify(off) refused: %s" % lib().stm_last_error().decode())
            return
        from . import rectify as _rectify
        rec = np.ascontiguousarray(np.stack([_rectify.check(rec_l, "left record"), _rectify.check(rec_r, "right record")]), dtype=np.float32)
        if int(lib().stm_stream_rectify(self._h, 1, rec.ctypes.data_as(C.POINTER(C.c_float)), int(border))) != 0:
            raise ValueError("stm_stream_rectify(border %d) refused: %s" % (border, lib().stm_last_error().decode()))

    def get_rectify(self):
        """stm_stream_get_rectify: None with the rectification off, else (rec_l, rec_r, border)."""
        mode, border = C.c_int(0), C.c_int(0)
        rec = np.zeros((2, 18), np.float32)
        lib().stm_stream_get_rectify(self._h, C.byref(mode), rec.ctypes.data_as(C.POINTER(C.c_float)), C.byref(border))
        return None if mode.value == 0 else (rec[0], rec[1], border.value)

    def depth_frame_bytes(self):
        """(the plane's byte offset in a depth frame, the frame's bytes): the image's bytes rounded up to a multiple of 16, and that
        plus the tight plane"""
        assert self._depth_input is not None
        off = (self.H * self.Wsbs * 3 + 15) // 16 * 16
        return off, off + self.H * self.W * self._depth_input.itemsize

    def pack_depth_frame(self, img, plane):
        """The flat frame of a stream with depth input: the image uint8 [H][Wsbs][3], then the plane [H][W] of the stream's format at
        the next multiple of 16 bytes.  Returns a uint8 array of depth_frame_bytes()[1] bytes."""
        off, n = self.depth_frame_bytes()
        img = np.ascontiguousarray(img, dtype=np.uint8)
        plane = np.asarray(plane)
        if img.shape != self.in_shape or plane.shape != (self.H, self.W) or plane.dtype != self._depth_input:
            raise ValueError("a depth frame is an image uint8 %s and a plane %s %s, got %s %s and %s %s"
                             % (self.in_shape, self._depth_input, (self.H, self.W), img.dtype, img.shape, plane.dtype, plane.shape))
        flat = np.zeros(n, np.uint8)
        flat[:img.size] = img.reshape(-1)
        flat[off:] = np.ascontiguousarray(plane).view(np.uint8).reshape(-1)
        return flat

    def submit_depth(self, img, plane):
        """submit() for a stream with depth input: one image and its plane"""
        flat = self.pack_depth_frame(img, plane)
        return int(lib().stm_stream_submit(self._h, flat.ctypes.data_as(u8p)))

    def set_maps(self, format="f32", which="both", lo=0.0, hi=0.0):
        """stm_stream_maps: what a frame's disparity maps come back as -- "f32", "none", "u8" or "u16" (or 0 .. 3); for the planes
        `which` = "left", "right" or "both" (or 0, 1, 2) and the map values lo and hi of code 0 and of the largest code.  Only before
        the first submit.  Raises ValueError where the library refuses."""
        fmt = {"f32": 0, "none": 1, "u8": 2, "u16": 3}.get(format, format)
        sel = {"left": 0, "right": 1, "both": 2}.get(which, which)
        if not isinstance(fmt, int) or not isinstance(sel, int):
            raise ValueError("FrameStream.set_maps: format %r, which %r" % (format, which))
        if int(lib().stm_stream_maps(self._h, fmt, sel, float(lo), float(hi))) != 0:
            raise ValueError("stm_stream_maps(%r, %r, %g, %g) refused: %s" % (format, which, lo, hi, lib().stm_last_error().decode()))
        self._maps = (fmt, sel if fmt >= 2 else 2)

    def set_active(self, mode, rect=None, fill=0, fill_disp=0.0, thresh_luma=ACTIVE_AUTO_DEFAULT[0], lit_permille=ACTIVE_AUTO_DEFAULT[1],
                   max_bar_permille=ACTIVE_AUTO_DEFAULT[2], hold=ACTIVE_AUTO_DEFAULT[3]):
        """stm_stream_set_active: the active picture area of the stream's frames (device_api.set_active's and set_active_auto's
        arguments; the state is the stream's own); only before the first submit.  Raises ValueError where the library refuses."""
        r = None if rect is None else (C.c_int * 4)(*[int(v) for v in rect])
        if int(lib().stm_stream_set_active(self._h, int(mode), r, int(fill), float(fill_disp), int(thresh_luma), int(lit_permille),
                                           int(max_bar_permille), int(hold))) != 0:
            raise ValueError("stm_stream_set_active(%d, %r, %d, %g, %d, %d, %d, %d) refused: %s"
                             % (mode, rect, fill, fill_disp, thresh_luma, lit_permille, max_bar_permille, hold, lib().stm_last_error().decode()))

    def active(self):
        """stm_stream_active: (top, bottom, left, right, changed) of the most recently collected frame (the whole frame and 0 with
        the setting off), or None before the first collect."""
        out = (C.c_int * 5)()
        if int(lib().stm_stream_active(self._h, out)) != 0:
            return None
        return tuple(int(v) for v in out)

    def set_cut(self, mode, thresh_permille=CUT_DEFAULT[0], min_gap=CUT_DEFAULT[1]):
        """stm_stream_set_cut: the shot-change detector of the stream's frames (device_api.set_cut's arguments; the state is the
        stream's own); only before the first submit.  Raises ValueError where the library refuses."""
        if int(lib().stm_stream_set_cut(self._h, int(mode), int(thresh_permille), int(min_gap))) != 0:
            raise ValueError("stm_stream_set_cut(%d, %d, %d) refused: %s" % (mode, thresh_permille, min_gap, lib().stm_last_error().decode()))

    def cut(self):
        """stm_stream_cut: (cut, score, since) of the most recently collected frame ((0, 0, 0) with the detector off), or None
        before the first collect."""
        out = (C.c_int * 3)()
        if int(lib().stm_stream_cut(self._h, out)) != 0:
            return None
        return int(out[0]), int(out[1]), int(out[2])

    def set_balance(self, mode, lut=None):
        """stm_stream_set_balance: the colour balance of the stream's frames (device_api.set_balance's arguments); the stream's
        own, independent of the calling thread's; only before the first submit.  Raises ValueError where the library refuses."""
        buf = None
        if lut is not None:
            a = np.ascontiguousarray(lut)
            if a.dtype != np.uint8 or a.size != 768:
                raise ValueError("a balance table is 768 bytes of uint8 (B, G, R, 256 each), got %s %s" % (a.dtype, a.shape))
            buf = (C.c_uint8 * 768).from_buffer_copy(a.tobytes())
        if int(lib().stm_stream_set_balance(self._h, int(mode), buf)) != 0:
            raise ValueError("stm_stream_set_balance(%d) refused: %s" % (mode, lib().stm_last_error().decode()))

    def set_balance_auto(self, max_shift=48, rate=1.0):
        """stm_stream_set_balance_auto: mode 2's parameters (device_api.set_balance_auto's; the state is the stream's own); only
        before the first submit.  Raises ValueError where the library refuses."""
        if int(lib().stm_stream_set_balance_auto(self._h, int(max_shift), float(rate))) != 0:
            raise ValueError("stm_stream_set_balance_auto(%d, %g) refused: %s" % (max_shift, rate, lib().stm_last_error().decode()))

    def balance(self):
        """stm_stream_balance: the (3, 256) uint8 tables applied to the most recently collected frame, or None before the first
        collect."""
        out = (C.c_uint8 * 768)()
        if int(lib().stm_stream_balance(self._h, out)) != 0:
            return None
        return np.frombuffer(bytes(out), np.uint8).reshape(3, 256).copy()

    def set_align(self, mode, a=0.0, b=0.0, c=0.0):
        """stm_stream_set_align: the vertical alignment of the stream's frames (device_api.set_align's arguments); the stream's
        own, independent of the calling thread's; only before the first submit.  Raises ValueError where the library refuses."""
        if int(lib().stm_stream_set_align(self._h, int(mode), float(a), float(b), float(c))) != 0:
            raise ValueError("stm_stream_set_align(%d, %g, %g, %g) refused: %s" % (mode, a, b, c, lib().stm_last_error().decode()))

    def set_align_auto(self, radius=16, rate=1.0):
        """stm_stream_set_align_auto: mode 2's parameters (device_api.set_align_auto's; the state is the stream's own); only before
        the first submit.  Raises ValueError where the library refuses."""
        if int(lib().stm_stream_set_align_auto(self._h, int(radius), float(rate))) != 0:
            raise ValueError("stm_stream_set_align_auto(%d, %g) refused: %s" % (radius, rate, lib().stm_last_error().decode()))

    def align(self):
        """stm_stream_align: (a, b, c) applied to the most recently collected frame, or None before the first collect."""
        out = (C.c_float * 3)()
        if int(lib().stm_stream_align(self._h, C.cast(out, f32p))) != 0:
            return None
        return float(out[0]), float(out[1]), float(out[2])

    def set_antialias(self, mode, strength=1.0, max_radius=8, gate=1.0):
        """stm_stream_set_antialias: the view antialiasing of the stream's frames (device_api.set_antialias's arguments); the
        stream's own, independent of the calling thread's; only before the first submit.  Raises ValueError where the library
        refuses."""
        if int(lib().stm_stream_set_antialias(self._h, int(mode), float(strength), int(max_radius), float(gate))) != 0:
            raise ValueError("stm_stream_set_antialias(%d, %g, %d, %g) refused: %s"
                             % (mode, strength, max_radius, gate, lib().stm_last_error().decode()))

    def set_overlay(self, max_rows=0, max_cols=0):
        """stm_stream_set_overlay: room for overlays of up to max_rows x max_cols pixels; (0, 0) = off.  Only before the first
        submit; refused together with an NV12 output.  Raises ValueError where the library refuses."""
        if int(lib().stm_stream_set_overlay(self._h, int(max_rows), int(max_cols))) != 0:
            raise ValueError("stm_stream_set_overlay(%d, %d) refused: %s" % (max_rows, max_cols, lib().stm_last_error().decode()))

    def set_overlay_auto(self, mode, limit_lo=0.0, limit_hi=0.0, near_permille=20, margin=1.0, pad=8, rate_near=1.0, rate_far=0.1):
        """stm_stream_set_overlay_auto: the automatic placement of the stream's overlay (device_api.set_overlay_auto's parameters;
        the state is the stream's own); only before the first submit and after set_overlay.  Raises ValueError where the library
        refuses."""
        if int(lib().stm_stream_set_overlay_auto(self._h, int(mode), int(near_permille), float(margin), int(pad), float(limit_lo),
                                                 float(limit_hi), float(rate_near), float(rate_far))) != 0:
            raise ValueError("stm_stream_set_overlay_auto(%d, %d, %g, %d, %g, %g, %g, %g) refused: %s"
                             % (mode, near_permille, margin, pad, limit_lo, limit_hi, rate_near, rate_far, lib().stm_last_error().decode()))

    def overlay_depth(self):
        """stm_stream_overlay_depth: the overlay's state (valid, disparity, nearest, 0) as the most recently collected frame left it
        -- a float32 array of four -- or None before the first collect."""
        out = (C.c_float * 4)()
        if int(lib().stm_stream_overlay_depth(self._h, C.cast(out, f32p))) != 0:
            return None
        return np.array(list(out), np.float32)

    def overlay(self, bgra, x0=0, y0=0, disparity=0.0):
        """stm_stream_overlay: the overlay every later submit composites, until the next call -- uint8 [rows][cols][4], B, G, R, A
        with premultiplied alpha (premultiply converts straight alpha), its top-left corner at view pixel (x0, y0), at the
        end-to-end `disparity` (> 0 behind the screen, < 0 in front) -- or None = none.  Callable between any two submits; the
        array is reusable on return.  Raises ValueError where the library refuses."""
        if bgra is None:
            r = lib().stm_stream_overlay(self._h, None, 0, 0, 0, 0, 0.0)
        else:
            bgra = np.ascontiguousarray(bgra, dtype=np.uint8)
            assert bgra.ndim == 3 and bgra.shape[2] == 4
            r = lib().stm_stream_overlay(self._h, bgra.ctypes.data_as(u8p), bgra.shape[0], bgra.shape[1], int(x0), int(y0), float(disparity))
        if int(r) != 0:
            raise ValueError("stm_stream_overlay refused: %s" % lib().stm_last_error().decode())

    def set_depth(self, mode, gain=1.0, conv=0.0):
        """stm_stream_set_depth: the depth budget of the stream's frames (device_api.set_depth's arguments); the stream's own,
        independent of the calling thread's; only before the first submit.  Mode 2 needs set_depth_auto first.  Raises ValueError
        where the library refuses."""
        if int(lib().stm_stream_set_depth(self._h, int(mode), float(gain), float(conv))) != 0:
            raise ValueError("stm_stream_set_depth(%d, %g, %g) refused: %s" % (mode, gain, conv, lib().stm_last_error().decode()))

    def set_depth_auto(self, disp_lo, disp_hi, max_gain=1.0, clip_permille=20, rate=1.0):
        """stm_stream_set_depth_auto: mode 2's parameters (device_api.set_depth_auto's; the state is the stream's own); only before
        the first submit.  Raises ValueError where the library refuses."""
        if int(lib().stm_stream_set_depth_auto(self._h, float(disp_lo), float(disp_hi), float(max_gain), int(clip_permille),
                                               float(rate))) != 0:
            raise ValueError("stm_stream_set_depth_auto(%g, %g, %g, %d, %g) refused: %s"
                             % (disp_lo, disp_hi, max_gain, clip_permille, rate, lib().stm_last_error().decode()))

    def depth(self):
        """stm_stream_depth: (gain, conv) applied to the most recently collected frame, or None before the first collect."""
        out = (C.c_float * 2)()
        if int(lib().stm_stream_depth(self._h, C.cast(out, f32p))) != 0:
            return None
        return float(out[0]), float(out[1])

    def set_lens(self, mode, pitch=0.0, slope=0.0, centre=0.0):
        """stm_stream_set_lens: the display geometry the stream's frames are interlaced through (device_api.set_lens's arguments);
        the stream's own, independent of the calling thread's; only before the first submit.  Raises ValueError where the library
        refuses."""
        if int(lib().stm_stream_set_lens(self._h, int(mode), float(pitch), float(slope), float(centre))) != 0:
            raise ValueError("stm_stream_set_lens(%d, %g, %g, %g) refused: %s"
                             % (mode, pitch, slope, centre, lib().stm_last_error().decode()))

    def set_layout(self, layout=0, tiles_x=1, tiles_y=1, order=0, filter=0):
        """stm_stream_set_layout: the output geometry of the stream's frames (device_api.set_layout's arguments); the stream's own,
        independent of the calling thread's; only before the first submit.  Raises ValueError where the library refuses."""
        if int(lib().stm_stream_set_layout(self._h, int(layout), int(tiles_x), int(tiles_y), int(order), int(filter))) != 0:
            raise ValueError("stm_stream_set_layout(%d, %d, %d, %d, %d) refused: %s"
                             % (layout, tiles_x, tiles_y, order, filter, lib().stm_last_error().decode()))

    def set_output(self, format=0, matrix=0):
        """stm_stream_set_output: the format of the stream's output frames, 0 = BGR [out_rows][out_cols][3], 1 = NV12
        [out_rows * 3 / 2][out_cols] converted by `matrix` (quilts only: set the layout first); the stream's own, independent of the
        calling thread's; only before the first submit.  Raises ValueError where the library refuses."""
        if int(lib().stm_stream_set_output(self._h, int(format), int(matrix))) != 0:
            raise ValueError("stm_stream_set_output(%d, %d) refused: %s" % (format, matrix, lib().stm_last_error().decode()))
        self.out_shape = (self.Ho * 3 // 2, self.Wo) if int(format) == 1 else (self.Ho, self.Wo, 3)

    def set_input(self, input_format, matrix=0):
        """stm_stream_set_input: "bgr" or "nv12" with its conversion matrix; only before the first submit.  Raises ValueError where
        the library refuses."""
        fmt = {"bgr": 0, "nv12": 1}.get(input_format, -1)
        if int(lib().stm_stream_set_input(self._h, fmt, int(matrix))) != 0:
            raise ValueError("stm_stream_set_input(%r, %d) refused: %s" % (input_format, matrix, lib().stm_last_error().decode()))
        self._nv12 = fmt == 1
        self.in_shape = (self.rows_f * 3 // 2, self.Wsbs) if fmt == 1 else (self.rows_f, self.Wsbs, 3)

    def set_packing(self, packing=0, swap=0, filter=0, gap=0):
        """stm_stream_set_packing: the packing of the stream's input frames; the stream's own, independent of the calling thread's;
        only before the first submit.  The frame's row length was fixed when the stream was created (the `packing` argument of the
        constructor sizes it), so this is for changing swap or filter, or for a stream created with that row length.  Buffers handed
        out by input_buffer() before this call are void.  Raises ValueError where the library refuses."""
        if int(lib().stm_stream_set_packing(self._h, int(packing), int(swap), int(filter), int(gap))) != 0:
            raise ValueError("stm_stream_set_packing(%d, %d, %d, %d) refused: %s"
                             % (packing, swap, filter, gap, lib().stm_last_error().decode()))
        self.packing = (int(packing), int(swap), int(filter), int(gap))
        self.rows_f = packed_frame_geometry(self.H, self.W, self.packing)[1]
        self.in_shape = (self.rows_f * 3 // 2, self.Wsbs) if self._nv12 else (self.rows_f, self.Wsbs, 3)

    def set_match_size(self, num_rows_disp=0, num_cols_disp=0, disp_scale=1.0):
        """stm_stream_set_match_size: the size the stream's frames are matched at and the reduced frame's disp_scale; (0, 0) = off,
        the full-resolution frame.  Only before the first submit.  Raises ValueError where the library refuses."""
        if int(lib().stm_stream_set_match_size(self._h, int(num_rows_disp), int(num_cols_disp), float(disp_scale))) != 0:
            raise ValueError("stm_stream_set_match_size(%d, %d, %g) refused: %s"
                             % (num_rows_disp, num_cols_disp, disp_scale, lib().stm_last_error().decode()))

    def set_stages(self, stages):
        """stm_stream_set_stages: 3, optionally OR-ed with 0x200 (sub-pixel), 0x400 (outlier interpolation), 0x800 (linear
        sampling of the views' warps), 0x2000 (temporal stabilisation of the maps against the previous frame's) and -- with a match
        size -- 0x1000 (guided up-sampling of the maps); only before
        the first submit.  Raises ValueError where the library refuses (it returns -1; in error mode 0 it exits like any error)."""
        if int(lib().stm_stream_set_stages(self._h, int(stages))) != 0:
            raise ValueError("stm_stream_set_stages(%#x) refused: %s" % (stages, lib().stm_last_error().decode()))

    def set_temporal(self, alpha=0.5, thresh_color=24, thresh_disp=1.5):
        """stm_stream_set_temporal: the parameters of the temporal step (stages bit 0x2000); only before the first submit.
        Raises ValueError where the library refuses."""
        if int(lib().stm_stream_set_temporal(self._h, float(alpha), int(thresh_color), float(thresh_disp))) != 0:
            raise ValueError("stm_stream_set_temporal(%g, %d, %g) refused: %s"
                             % (alpha, thresh_color, thresh_disp, lib().stm_last_error().decode()))

    def submit(self, sbs):
        sbs = np.ascontiguousarray(sbs, dtype=np.uint8)
        if self._depth_input is not None:  # the flat frame pack_depth_frame returns
            assert sbs.shape == (self.depth_frame_bytes()[1],)
            return int(lib().stm_stream_submit(self._h, sbs.ctypes.data_as(u8p)))
        assert sbs.shape == self.in_shape
        return int(lib().stm_stream_submit(self._h, sbs.ctypes.data_as(u8p)))

    def input_buffer(self):
        """The pinned buffer the next submit() will use, as an (H, 2W, 3) uint8 view -- (H * 3 / 2, 2W) in NV12 mode -- or None
        while that slot is uncollected: write the frame into it and call submit_inplace() -- no host copy."""
        p = lib().stm_stream_input_buffer(self._h)
        if not p:
            return None
        if self._depth_input is not None:  # flat: the image, then the plane at depth_frame_bytes()[0]
            return np.ctypeslib.as_array(C.cast(p, u8p), shape=(self.depth_frame_bytes()[1],))
        return np.ctypeslib.as_array(C.cast(p, u8p), shape=self.in_shape)

    def submit_inplace(self):
        return int(lib().stm_stream_submit(self._h, None))

    def collect_view(self):
        """Like collect(), but returns views of the stream's pinned result buffers (valid until the frame after the next
        one is submitted) instead of copies."""
        if self._maps[0] != 0:  # planes, or no maps: uint8 / uint16 views, None for a plane the stream does not produce
            vl, vr, po = C.c_void_p(), C.c_void_p(), u8p()
            k = int(lib().stm_stream_collect_maps_view(self._h, C.byref(vl), C.byref(vr), C.byref(po)))
            if k < 0:
                return None
            ct = C.c_uint8 if self._maps[0] == 2 else C.c_uint16
            planes = [np.ctypeslib.as_array(C.cast(v, C.POINTER(ct)), shape=(self.H, self.W)) if v.value else None for v in (vl, vr)]
            return k, planes[0], planes[1], np.ctypeslib.as_array(po, shape=self.out_shape)
        pl, pr, po = f32p(), f32p(), u8p()
        k = int(lib().stm_stream_collect_view(self._h, C.byref(pl), C.byref(pr), C.byref(po)))
        if k < 0:
            return None
        return (k, np.ctypeslib.as_array(pl, shape=(self.H, self.W)), np.ctypeslib.as_array(pr, shape=(self.H, self.W)),
                np.ctypeslib.as_array(po, shape=self.out_shape))

    def collect(self):
        if self._maps[0] != 0:
            fmt, sel = self._maps
            dt = np.uint8 if fmt == 2 else np.dtype("<u2")
            dl = np.empty((self.H, self.W), dt) if fmt >= 2 and sel != 1 else None
            dr = np.empty((self.H, self.W), dt) if fmt >= 2 and sel != 0 else None
            out = np.empty(self.out_shape, np.uint8)
            k = int(lib().stm_stream_collect_maps(self._h, None if dl is None else dl.ctypes.data, None if dr is None else dr.ctypes.data,
                                                  out.ctypes.data_as(u8p)))
            return (k, dl, dr, out) if k >= 0 else None
        dl = np.empty((self.H, self.W), np.float32)
        dr = np.empty((self.H, self.W), np.float32)
        out = np.empty(self.out_shape, np.uint8)
        k = int(lib().stm_stream_collect(self._h, dl.ctypes.data_as(f32p), dr.ctypes.data_as(f32p), out.ctypes.data_as(u8p)))
        return (k, dl, dr, out) if k >= 0 else None

    def close(self):
        if self._h:
            lib().stm_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def premultiply(bgra_straight):
    """A straight-alpha overlay (uint8 [rows][cols][4], B, G, R, A) as the premultiplied one the library composites: each colour
    byte becomes (c * a + 127) // 255 -- never above its alpha, exact at a = 0 and a = 255."""
    a = np.asarray(bgra_straight, dtype=np.uint8)
    assert a.ndim == 3 and a.shape[2] == 4
    out = a.copy()
    alpha = a[..., 3:4].astype(np.uint32)
    out[..., :3] = ((a[..., :3].astype(np.uint32) * alpha + 127) // 255).astype(np.uint8)
    return out


def packed_frame_geometry(num_rows, num_cols, packing):
    """(Wsbs, rows_f) of the smallest frame that holds two eyes of num_rows x num_cols after unpacking (include/stm_hip.h,
    stm_demux_packed); packing = (packing, swap, filter, gap)"""
    pk, gap = int(packing[0]), int(packing[3])
    if pk == 0:
        return 2 * num_cols + gap, num_rows
    if pk == 1:
        return 2 * (num_cols // 2) + gap, num_rows
    if pk == 2:
        return num_cols, 2 * num_rows + gap
    return num_cols, 2 * (num_rows // 2) + gap


def unpacked_eye_shape(frame_rows, frame_cols, packing):
    """(num_rows, num_cols) of an unpacked eye of a packed frame that is exactly as large as packed_frame_geometry says"""
    pk, gap = int(packing[0]), int(packing[3])
    if pk < 2:
        return frame_rows, ((frame_cols - gap) // 2) * (2 if pk == 1 else 1)
    return ((frame_rows - gap) // 2) * (2 if pk == 3 else 1), frame_cols


def take_balance_options(argv):
    """The two drivers' --balance FILE.npy (768 bytes of uint8: B, G, R, 256 each) and --balance-auto [MAX_SHIFT RATE] (both numbers
    or neither: 48 and 1), removed from argv.  Returns (tables as a (3, 256) array or None, (max_shift, rate) or None); raises
    ValueError or IndexError for a malformed option, an unreadable or misshapen file, a value out of range, or both options."""
    balance, balance_auto = None, None
    if "--balance" in argv:
        at = argv.index("--balance")
        try:
            a = np.load(argv[at + 1], allow_pickle=False)
        except OSError as e:
            raise ValueError(str(e))
        if a.dtype != np.uint8 or a.size != 768:
            raise ValueError("--balance: %s holds %s %s, not 768 bytes of uint8" % (argv[at + 1], a.dtype, a.shape))
        balance = np.ascontiguousarray(a).reshape(3, 256)
        del argv[at:at + 2]
    if "--balance-auto" in argv:
        at = argv.index("--balance-auto")
        vals = []
        for tok in argv[at + 1:at + 3]:
            try:
                float(tok)
            except ValueError:
                break
            vals.append(tok)
        if len(vals) == 1:
            raise ValueError("--balance-auto takes MAX_SHIFT and RATE, or neither")
        balance_auto = (int(vals[0]), float(vals[1])) if vals else (48, 1.0)
        if not 0 <= balance_auto[0] <= 255 or not 0.0 < balance_auto[1] <= 1.0:
            raise ValueError(balance_auto)
        del argv[at:at + 1 + len(vals)]
    if balance is not None and balance_auto is not None:
        raise ValueError("--balance and --balance-auto")
    return balance, balance_auto


def take_cut_option(argv):
    """The driver's --cut [THRESH MIN_GAP] (both numbers or neither: CUT_DEFAULT), removed from argv.  Returns (thresh_permille,
    min_gap) or None; raises ValueError for a malformed option or a value out of range."""
    if "--cut" not in argv:
        return None
    at = argv.index("--cut")
    vals = []
    for tok in argv[at + 1:at + 3]:
        try:
            int(tok)
        except ValueError:
            break
        vals.append(tok)
    if len(vals) == 1:
        raise ValueError("--cut takes THRESH and MIN_GAP, or neither")
    cut = (int(vals[0]), int(vals[1])) if vals else CUT_DEFAULT
    if not 1 <= cut[0] <= 1000 or not 1 <= cut[1] <= (1 << 20):
        raise ValueError(cut)
    del argv[at:at + 1 + len(vals)]
    return cut


def take_active_options(argv):
    """The drivers' --active T B L R, --active-auto [THRESH LIT MAX_BAR HOLD] (all four numbers or none: ACTIVE_AUTO_DEFAULT) and
    --active-fill DISP, removed from argv.  Returns (rect or None, (thresh_luma, lit_permille, max_bar_permille, hold) or None,
    fill disparity or None); raises ValueError for a malformed option, a value out of range, both --active and --active-auto, or
    --active-fill without either."""
    rect, auto, fill = None, None, None
    if "--active" in argv:
        at = argv.index("--active")
        toks = argv[at + 1:at + 5]
        if len(toks) != 4:
            raise ValueError("--active takes T B L R")
        rect = tuple(int(t) for t in toks)
        if not (0 <= rect[0] < rect[1] and 0 <= rect[2] < rect[3]):
            raise ValueError(rect)
        del argv[at:at + 5]
    if "--active-auto" in argv:
        at = argv.index("--active-auto")
        vals = []
        for tok in argv[at + 1:at + 5]:
            try:
                int(tok)
            except ValueError:
                break
            vals.append(tok)
        if len(vals) not in (0, 4):
            raise ValueError("--active-auto takes THRESH LIT MAX_BAR HOLD, or none of them")
        auto = tuple(int(v) for v in vals) if vals else ACTIVE_AUTO_DEFAULT
        if not (0 <= auto[0] <= 254 and 0 <= auto[1] <= 999 and 0 <= auto[2] <= 450 and 1 <= auto[3] <= (1 << 20)):
            raise ValueError(auto)
        del argv[at:at + 1 + len(vals)]
    if "--active-fill" in argv:
        at = argv.index("--active-fill")
        if at + 1 >= len(argv):
            raise ValueError("--active-fill takes DISP")
        fill = float(argv[at + 1])
        if not abs(fill) <= 4096.0:  # a NaN fails the comparison
            raise ValueError(fill)
        del argv[at:at + 2]
    if rect is not None and auto is not None:
        raise ValueError("--active and --active-auto")
    if fill is not None and rect is None and auto is None:
        raise ValueError("--active-fill needs --active or --active-auto")
    return rect, auto, fill


DEPTH_INPUT_FORMATS = {np.dtype(np.float32): "f32", np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16"}


def take_depth_input_option(argv, stack=False):
    """The drivers' --depth-input PLANE.npy LO HI [FILL GATE] (both of FILL and GATE or neither: 0 and 0), removed from argv.  The file
    holds one plane [H][W] -- with `stack` a stack [n][H][W], one plane a frame -- of float32, uint8 or uint16, and the format follows
    the dtype.  Returns (planes, (format, lo, hi, fill, gate)) or None; raises ValueError or IndexError for a malformed option, an
    unreadable or misshapen file or a value stm_stream_input_depth would refuse."""
    if "--depth-input" not in argv:
        return None
    at = argv.index("--depth-input")
    path, lo, hi = argv[at + 1], float(argv[at + 2]), float(argv[at + 3])
    vals = []
    for tok in argv[at + 4:at + 6]:
        try:
            float(tok)
        except ValueError:
            break
        vals.append(tok)
    if len(vals) == 1:
        raise ValueError("--depth-input takes FILL and GATE, or neither")
    fill, gate = (int(vals[0]), float(vals[1])) if vals else (0, 0.0)
    if not (abs(lo) <= 4096.0 and abs(hi) <= 4096.0 and abs(hi - lo) >= 1.0 / 64.0) or fill not in (0, 1) or not 0.0 <= gate <= 4096.0:  # a NaN fails
        raise ValueError((lo, hi, fill, gate))
    try:
        planes = np.load(path, allow_pickle=False)
    except OSError as e:
        raise ValueError(str(e))
    if planes.dtype not in DEPTH_INPUT_FORMATS or planes.ndim != (3 if stack else 2):
        raise ValueError("--depth-input: %s holds %s %s, not %s of float32, uint8 or uint16"
                         % (path, planes.dtype, planes.shape, "a stack [n][H][W]" if stack else "a plane [H][W]"))
    del argv[at:at + 4 + len(vals)]
    return planes, (DEPTH_INPUT_FORMATS[planes.dtype], lo, hi, fill, gate)


def take_depth_video_option(argv):
    """The drivers' --depth-video RANGE DFILTER DGATE LO HI [FILL GATE] (both of FILL and GATE or neither: 0 and 0), removed from argv:
    the frames are packed 2D-plus-depth video frames whose layout the drivers' --nv12, --matrix and --packing options give.  Returns
    (range, dfilter, dgate, lo, hi, fill, gate) or None; raises ValueError or IndexError for a malformed option or a value
    stm_stream_input_packed_depth would refuse of these seven."""
    if "--depth-video" not in argv:
        return None
    at = argv.index("--depth-video")
    rng, dfilter, dgate = (int(v) for v in argv[at + 1:at + 4])
    lo, hi = float(argv[at + 4]), float(argv[at + 5])
    vals = []
    for tok in argv[at + 6:at + 8]:
        try:
            float(tok)
        except ValueError:
            break
        vals.append(tok)
    if len(vals) == 1:
        raise ValueError("--depth-video takes FILL and GATE, or neither")
    fill, gate = (int(vals[0]), float(vals[1])) if vals else (0, 0.0)
    if rng not in (0, 1) or dfilter not in (0, 1) or not 0 <= dgate <= 255 or fill not in (0, 1) or not 0.0 <= gate <= 4096.0:
        raise ValueError((rng, dfilter, dgate, fill, gate))
    if not (abs(lo) <= 4096.0 and abs(hi) <= 4096.0 and abs(hi - lo) >= 1.0 / 64.0):  # a NaN fails
        raise ValueError((lo, hi))
    del argv[at:at + 6 + len(vals)]
    return rng, dfilter, dgate, lo, hi, fill, gate


def take_rectify_option(argv):
    """The drivers' --rectify FILE.npy [BORDER] (BORDER 0 or 1, default 0), removed from argv.  The file is a (2, 18) float32 array:
    the left eye's rectification record, then the right eye's (stm_amd.rectify.record).  Returns (rec_l, rec_r, border) or None;
    raises ValueError or IndexError for a malformed option or file, before any frame is read."""
    if "--rectify" not in argv:
        return None
    from . import rectify as _rectify
    at = argv.index("--rectify")
    path = argv[at + 1]
    n, border = 2, 0
    if at + 2 < len(argv) and argv[at + 2] in ("0", "1"):
        n, border = 3, int(argv[at + 2])
    rec_l, rec_r = _rectify.load_records(path)
    del argv[at:at + n]
    return rec_l, rec_r, border


def take_maps_option(argv):
    """The driver's --maps FORMAT [WHICH LO HI [FILE]], removed from argv: FORMAT f32, none, u8 or u16; for u8 and u16 WHICH (left,
    right or both) and the map values LO and HI of code 0 and of the largest code, then optionally the FILE the raw planes are
    appended to (the next token, unless it starts with "--").  Returns (format, which, lo, hi, file or None) or None; raises ValueError
    or IndexError for a malformed option or a value stm_stream_maps would refuse."""
    if "--maps" not in argv:
        return None
    at = argv.index("--maps")
    fmt = argv[at + 1]
    if fmt in ("f32", "none"):
        del argv[at:at + 2]
        return fmt, "both", 0.0, 0.0, None
    if fmt not in ("u8", "u16"):
        raise ValueError("--maps FORMAT is f32, none, u8 or u16")
    which, lo, hi = argv[at + 2], float(argv[at + 3]), float(argv[at + 4])
    if which not in ("left", "right", "both") or not (abs(lo) <= 4096.0 and abs(hi) <= 4096.0 and abs(hi - lo) >= 1.0 / 64.0):  # a NaN fails
        raise ValueError((which, lo, hi))
    path = argv[at + 5] if at + 5 < len(argv) and not argv[at + 5].startswith("--") else None
    del argv[at:at + (6 if path is not None else 5)]
    return fmt, which, lo, hi, path


def _collect(fs, on_depth, on_align=None, on_balance=None, on_cut=None, on_overlay_depth=None, on_active=None):
    r = fs.collect()
    if on_active is not None and r is not None:
        on_active(r[0], fs.active())
    if on_overlay_depth is not None and r is not None:
        on_overlay_depth(r[0], fs.overlay_depth())
    if on_cut is not None and r is not None:
        on_cut(r[0], fs.cut())
    if on_balance is not None and r is not None:
        on_balance(r[0], fs.balance())
    if on_depth is not None and r is not None:
        on_depth(r[0], fs.depth())
    if on_align is not None and r is not None:
        on_align(r[0], fs.align())
    return r


def process_sequence(frames, params, out_rows=None, out_cols=None, stages=3, temporal=None, input_format="bgr", matrix=0, lens=None,
                     depth=None, depth_auto=None, on_depth=None, packing=None, eye_shape=None, layout=None, match=None, output=None,
                     overlay=None, antialias=None, align=None, align_auto=None, on_align=None, balance=None, balance_auto=None,
                     on_balance=None, cut=None, on_cut=None, overlay_auto=None, on_overlay_depth=None, active=None,
                     active_auto=None, active_fill=None, on_active=None, maps=None, depth_input=None, rectify=None, depth_video=None):
    """Generator: yields (index, disp_l, disp_r, interlaced) for every side-by-side frame of `frames`.
    depth_input: FrameStream's (format, lo, hi[, fill, gate]): `frames` then yields (image, plane) pairs, the image [H][W][3].
    depth_video: FrameStream's (format, matrix, packing, swap, filter, gap, range, dfilter, dgate, lo, hi[, fill, gate]): `frames` then
    yields packed 2D-plus-depth frames, BGR or NV12 by its format; eye_shape as under `packing`.
    maps: FrameStream's (format, which, lo, hi): disp_l and disp_r are then uint8 / uint16 depth planes, or None.
    input_format / matrix: FrameStream's ("nv12": the frames are [H * 3 / 2][2W] arrays, read_nv12_sequence's).
    stages: FrameStream.set_stages (3 | 0x200 sub-pixel | 0x400 outlier interpolation | 0x800 linear sampling | 0x2000 temporal
    stabilisation); temporal: (alpha, thresh_color, thresh_disp) for FrameStream.set_temporal, None = the defaults; lens: (mode,
    pitch, slope, centre) for FrameStream.set_lens, None = the reference's interlacer; depth / depth_auto: FrameStream's depth
    budget; on_depth: called with (index, (gain, conv)) after every collected frame.  packing: FrameStream's; the frames are then packed
    ones; eye_shape = (num_rows, num_cols), the size of an unpacked eye, defaults to what a frame without spare columns holds.
    layout: FrameStream's (the interlaced output is then a quilt).  match: FrameStream's (h, w, disp_scale): the reduced-resolution frame.
    output: FrameStream's (1, matrix): the quilt comes out as NV12, [out_rows * 3 / 2][out_cols].
    overlay: (bgra, x0, y0, disparity), one premultiplied overlay composited into every frame of the sequence (FrameStream.overlay).
    antialias: FrameStream's (strength, max_radius, gate): view antialiasing of every frame.  align / align_auto: FrameStream's
    vertical alignment of every frame's pair; on_align: called with (index, (a, b, c)) after every collected frame.  balance /
    balance_auto: FrameStream's colour balance of every frame's pair; on_balance: called with (index, tables) likewise.  cut:
    FrameStream's shot-change detector; on_cut: called with (index, (cut, score, since)) likewise.  overlay_auto: FrameStream's
    automatic placement of `overlay`, whose disparity is then ignored; on_overlay_depth: called with (index, state) likewise.
    active / active_auto / active_fill: FrameStream's active picture area; on_active: called with (index, (top, bottom, left, right,
    changed)) likewise.  rectify: FrameStream's (rec_l, rec_r[, border]): every frame's eyes remapped through their records first."""
    fs = None
    pending = 0
    for sbs in frames:
        if fs is None:
            first = sbs[0] if depth_input is not None else sbs
            nv12 = input_format == "nv12" or (depth_video is not None and depth_video[0] in ("nv12", 1))
            rows = first.shape[0] * 2 // 3 if nv12 else first.shape[0]
            cols = first.shape[1] if depth_input is not None else first.shape[1] // 2
            pitch = None
            if packing is not None:
                rows, cols = eye_shape if eye_shape is not None else unpacked_eye_shape(rows, sbs.shape[1], packing)
            elif depth_video is not None:
                rows, cols = eye_shape if eye_shape is not None else unpacked_eye_shape(rows, sbs.shape[1], tuple(depth_video[2:6]))
                pitch = sbs.shape[1]
            fs = FrameStream(rows, cols, params, out_rows, out_cols, stages, input_format, matrix, lens, depth, depth_auto, packing, layout, match, output,
                             overlay=None if overlay is None else tuple(np.asarray(overlay[0]).shape[:2]), antialias=antialias,
                             align=align, align_auto=align_auto, balance=balance, balance_auto=balance_auto, cut=cut, overlay_auto=overlay_auto,
                             active=active, active_auto=active_auto, active_fill=active_fill, maps=maps, depth_input=depth_input, rectify=rectify,
                             depth_video=depth_video, depth_pitch=pitch)
            if overlay is not None:
                fs.overlay(*overlay)
            if temporal is not None:
                fs.set_temporal(*temporal)
        if pending == 2:
            yield _collect(fs, on_depth, on_align, on_balance, on_cut, on_overlay_depth, on_active)
            pending -= 1
        if depth_input is not None:
            fs.submit_depth(*sbs)
        else:
            fs.submit(sbs)
        pending += 1
    while fs is not None and pending:
        yield _collect(fs, on_depth, on_align, on_balance, on_cut, on_overlay_depth, on_active)
        pending -= 1
    if fs is not None:
        fs.close()


def read_bmp_sequence(directory, pattern="*.bmp"):
    for path in sorted(glob.glob(os.path.join(directory, pattern))):
        yield bmp_io.read_bmp(path)


def read_nv12_sequence(path, num_rows, num_cols_sbs):
    """The frames of a raw .yuv file of concatenated NV12 frames (num_rows x num_cols_sbs luma, no padding), each as a uint8
    [num_rows * 3 / 2][num_cols_sbs] array: the Y plane, then the interleaved UV plane.  A trailing partial frame is an error."""
    assert num_rows % 2 == 0 and num_cols_sbs % 2 == 0
    n = num_rows * num_cols_sbs * 3 // 2
    with open(path, "rb") as f:
        while True:
            buf = f.read(n)
            if not buf:
                return
            if len(buf) != n:
                raise ValueError("%s: %d trailing bytes are no whole %d x %d NV12 frame" % (path, len(buf), num_cols_sbs, num_rows))
            yield np.frombuffer(buf, np.uint8).reshape(num_rows * 3 // 2, num_cols_sbs)


def normalize_minmax_u8(a):
    """cv::normalize(src, dst, 0, 1, CV_MINMAX) followed by the 8-bit display scaling the viewer applies."""
    lo, hi = float(a.min()), float(a.max())
    if hi <= lo:
        return np.zeros(a.shape, np.uint8)
    return np.clip((a - lo) / (hi - lo) * 255.0, 0, 255).astype(np.uint8)


def write_outputs(out_dir, index, disp_l, disp_r, interlaced):
    os.makedirs(out_dir, exist_ok=True)
    bmp_io.write_bmp(os.path.join(out_dir, "interlaced_%05d.bmp" % index), interlaced)
    write_disparities(out_dir, index, disp_l, disp_r)


def write_disparities(out_dir, index, disp_l, disp_r):
    os.makedirs(out_dir, exist_ok=True)
    bmp_io.write_bmp(os.path.join(out_dir, "disp_l_%05d.bmp" % index), normalize_minmax_u8(disp_l))
    bmp_io.write_bmp(os.path.join(out_dir, "disp_r_%05d.bmp" % index), normalize_minmax_u8(disp_r))
