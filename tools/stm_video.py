#!/usr/bin/env python
"""Headless counterpart of the reference's video driver (video_io.cpp): same positional parameters, a directory of
side-by-side BMP frames instead of a video file, BMP outputs instead of a window.

usage: stm_video.py <frames dir> <num views> <angle> <out width> <out height> <num disp> <zero disp> <ad coeff>
                    <census coeff> <ucd> <lcd> <usd> <lsd> <thresh_s> <thresh_h> [out dir] [--interp] [--subpixel] [--linear-warp]
                    [--temporal [--temporal-alpha A] [--temporal-color C] [--temporal-disp T]]
                    [--nv12 ROWS COLS_SBS [--matrix M]] [--lens MODE PITCH SLOPE CENTRE]
                    [--depth GAIN CONV | --depth-auto LO HI [MAX_GAIN CLIP RATE]]
                    [--packing P SWAP FILTER GAP] [--quilt TX TY ORDER FILTER [--nv12-out MATRIX]] [--match H W SCALE [--guided-up]]
                    [--overlay FILE.npy X0 Y0 DISPARITY] [--overlay-auto LO HI [NEAR MARGIN PAD RATE_NEAR RATE_FAR]] [--antialias STRENGTH MAX_RADIUS GATE]
                    [--align A B C | --align-auto RADIUS [RATE]] [--balance FILE.npy | --balance-auto [MAX_SHIFT RATE]]
                    [--cut [THRESH MIN_GAP]]
                    [--active T B L R | --active-auto [THRESH LIT MAX_BAR HOLD]] [--active-fill DISP]
                    [--maps FORMAT [WHICH LO HI [FILE]]] [--depth-input PLANES.npy LO HI [FILL GATE]]
                    [--depth-video RANGE DFILTER DGATE LO HI [FILL GATE]]
                    [--rectify FILE.npy [BORDER]]
(the 15 arguments of video_io.cpp:49-109; frames are *.bmp, sorted by name)
--interp / --subpixel (additions, off by default): frame bits 0x400 (outlier interpolation after region voting) and 0x200
(sub-pixel enhancement) of every frame, set on the frame stream before its first frame.
--linear-warp (an addition, off by default): frame bit 0x800, the views' warps fetched at the fractional coordinate.
--temporal (an addition, off by default): frame bit 0x2000, every frame's maps stabilised against the previous frame's where
neither colour nor disparity moved; --temporal-alpha (0.5), --temporal-color (24) and --temporal-disp (1.5) set its parameters.
--nv12 ROWS COLS_SBS (an addition): <frames dir> is instead one raw .yuv file of concatenated side-by-side NV12 frames of ROWS rows
and COLS_SBS columns, converted on the GPU inside the frame's first kernel; --matrix M (0) picks the conversion: 0 / 1 = BT.601 /
BT.709 limited range, 2 / 3 = BT.601 / BT.709 full range.
--lens MODE PITCH SLOPE CENTRE (an addition): the panel's calibration (stm_set_lens) -- PITCH sub-pixels per lens, SLOPE sub-pixels
of lens shift per output row, CENTRE lenses of phase offset; MODE 1 = nearest view, 2 = two views blended, 3 = every sub-pixel
rendered at its own continuous position.  Replaces the reference's interlacer; <angle> is then ignored.
--depth GAIN CONV (an addition): the manual depth budget (stm_set_depth mode 1) -- a scene point of disparity d is shown with
GAIN * d - CONV (GAIN in [0, 8]; CONV in input-view pixels, |CONV| <= 4096).  --depth-auto LO HI [MAX_GAIN CLIP RATE]: the automatic
one (mode 2) -- every frame's disparity range, less CLIP/1000 of its pixels at either end (20), is brought into the panel's budget
[LO, HI] with a gain of at most MAX_GAIN (1), following the fit at RATE (1); each frame's applied pair is printed.  The two
options are mutually exclusive.
--packing P SWAP FILTER GAP (an addition): the frames are packed stereo frames (stm_set_packing) -- P 0 / 1 = side by side full /
half width, 2 / 3 = top and bottom full / half height; SWAP 1 = the right eye first; FILTER 0 = linear, 1 = Catmull-Rom (how a
squeezed eye is expanded); GAP pixels between the eyes (45 blank rows in 1080p HDMI frame packing).  Unpacked inside the frame's first
kernel; combines with --nv12, whose ROWS and COLS_SBS are then the packed frame's.  The frames carry no spare columns.
--quilt TX TY ORDER FILTER (an addition): the output frame is a quilt (stm_set_layout) -- the <num views> = TX * TY views whole, as
TX x TY tiles, instead of interlaced; ORDER bit 0 = tile rows bottom-up, bit 1 = tile 0 holds the leftmost camera (3 = the Looking
Glass convention); FILTER 0 = the reference's four-neighbour sampler, 1 = the area average.  <angle> is then ignored; excludes --lens.
--nv12-out MATRIX (an addition; needs --quilt): the quilt leaves the GPU as NV12 (stm_set_output), what a video encoder takes --
converted by MATRIX (as --matrix) inside the kernel that renders it -- and every frame is appended, raw, to <out dir>/quilt.yuv (a
file from an earlier run is replaced) instead of being written as a BMP; <out width> and <out height> and the tiles must be even.
--match H W SCALE (an addition): every frame is the reduced-resolution frame (stm_stream_set_match_size) -- the pair is matched at
H x W, the maps are scaled up by 1 / SCALE and the views rendered at full size; <num disp> and <zero disp> then count pixels of the
reduced pair.  --guided-up adds frame bit 0x1000, the guided up-sampler in place of the bilinear up-scale.  Excludes --packing.
--overlay FILE.npy X0 Y0 DISPARITY (an addition): FILE.npy holds one overlay, uint8 [rows][cols][4] -- B, G, R, A with premultiplied
alpha (video.premultiply converts straight alpha) -- composited into every frame of the sequence with its top-left corner at view pixel
(X0, Y0) -- a pixel of the frame, or of every tile under --quilt -- and at the end-to-end DISPARITY in pixels: > 0 behind the screen,
< 0 in front, 0 on it (stm_stream_overlay).  Excludes --nv12-out.
--overlay-auto LO HI [NEAR MARGIN PAD RATE_NEAR RATE_FAR] (an addition, used with --overlay, whose DISPARITY is then ignored): the
overlay's disparity is fitted on every frame on the GPU (stm_stream_set_overlay_auto) -- the NEAR permille (0 .. 499) nearest of both
maps' values under the overlay's opaque part, widened by PAD view pixels (0 .. 4096), as the views display it, MARGIN pixels nearer,
kept within [LO, HI]; a scene that comes nearer is followed at RATE_NEAR, one that recedes at RATE_FAR (both in (0, 1]).  The five
optional values default to 20, 1, 8, 1 and 0.1: choices, not measurements.  The disparity applied to each frame is printed.
--antialias STRENGTH MAX_RADIUS GATE (an addition): view antialiasing (stm_stream_set_antialias) -- before the views are rendered both
images are blurred along their rows by a box of 1 + STRENGTH * |displayed disparity| / (<num views> - 1) pixels (STRENGTH in [0, 8],
1 = one view spacing), at most MAX_RADIUS (1 .. 16) pixels to a side, using only neighbours whose disparity lies within GATE (>= 0) of
the pixel's own.  Content on the screen plane stays byte-identical; combines with every other option.
--align A B C (an addition): the vertical alignment of every frame's pair ahead of the matcher (stm_stream_set_align mode 1) -- the
right eye is sampled at row y + A + B u + C v, u and v counted from the centre of an eye: A rows of constant offset (a pitch
difference between the lenses), B rows per column (roll), C rows per row (focal length).  --align-auto RADIUS [RATE]: the field is
measured on every frame on the GPU within +-RADIUS rows (1 .. 32) and followed at RATE (1); each frame's applied field is printed.
The two options are mutually exclusive; both combine with every input format and every other option.
--balance FILE.npy (an addition): the colour balance between the eyes (stm_stream_set_balance mode 1) -- the right eye of every
frame goes through the three tables of FILE.npy (768 bytes of uint8: B, G, R, 256 each) ahead of the matcher, after the alignment.
--balance-auto [MAX_SHIFT RATE]: the tables are fitted on every frame on the GPU from the two eyes' histograms, moving no level by
more than MAX_SHIFT (0 .. 255; 48) and followed at RATE (1); each frame's tables are printed at the levels 64, 128 and 192.  The
two options are mutually exclusive; both combine with every input format and every other option.
--cut [THRESH MIN_GAP] (an addition): the shot-change detector (stm_stream_set_cut) -- every frame's left eye is compared on the GPU
with the previous frame's through a 4 x 4 grid of 16-bin luma histograms; a frame that scores THRESH permille (1 .. 1000; 370) or
more, at least MIN_GAP frames (3) after the last cut, is a cut, and the --depth-auto, --align-auto and --balance-auto states start
afresh on it.  Each frame's flag and score are printed, and at the end the indices of the frames found to be cuts.
--active T B L R (an addition): the picture's rectangle inside a letterboxed or pillarboxed frame (stm_stream_set_active mode 1) --
rows [T, B) and columns [L, R) of one eye; --depth-auto and --overlay-auto are then fitted under it, not under the bars.
--active-auto [THRESH LIT MAX_BAR HOLD]: the rectangle is measured on every frame's left eye on the GPU (mode 2) -- a line is picture
when more than LIT permille (0 .. 999; 10) of its pixels have a luma above THRESH (0 .. 254; 24); a bar is at most MAX_BAR permille
(0 .. 450; 300) of the frame to a side, grows only after HOLD (1 .. 2^20; 12) agreeing frames, shrinks at once, and starts afresh at a
--cut; each frame's rectangle is printed.  The two options are mutually exclusive.  --active-fill DISP (with either): the maps come
back with DISP (|DISP| <= 4096) in the bars.
--maps FORMAT [WHICH LO HI [FILE]] (an addition; put it behind the positional arguments): what the disparity maps leave the GPU as
(stm_stream_maps) -- FORMAT f32 (the default: float maps, written as normalised BMPs), none (no maps are downloaded or written), u8 or
u16: depth planes of one code per pixel of the maps WHICH selects (left, right or both), code 0 at map value LO and the largest code
at HI (LO > HI: near = dark; both within +-4096, at least 1/64 apart).  Every frame's planes -- raw, tight, u16 little-endian, the
left one first -- are appended to FILE (default <out dir>/maps_u8.raw or maps_u16.raw).
--depth-input PLANES.npy LO HI [FILL GATE] (an addition; put it behind the positional arguments): the frames of <frames dir> are single
images, the left eye, and PLANES.npy holds their depth planes, a stack [n][H][W] of float32, uint8 or uint16 (the format follows the
dtype; stm_stream_input_depth): disparities x_right - x_left, code 0 at LO and the largest code at HI (float32: clamped to the two).
The second eye is synthesised on the GPU and nothing is matched; FILL 0 (the default) extends the background into the disoccluded
holes, FILL 1 continues it from the mirror pixel where that lies within GATE of the background.  The matching parameters are read and
ignored; excludes --nv12, --packing, --match, --align, --balance and the frame bits other than --linear-warp.
--depth-video RANGE DFILTER DGATE LO HI [FILL GATE] (an addition; put it behind the positional arguments): the frames are packed
2D-plus-depth video frames (stm_stream_input_packed_depth): the image in one half and its depth, a grey picture, in the other.  The
frame's layout comes from the existing options: BGR files, or with --nv12 ROWS COLS_SBS [--matrix M] a raw NV12 file; --packing P SWAP
FILTER GAP says where the halves lie (the image is the first one unless SWAP is 1; FILTER expands a squeezed image; without it: side
by side, full size).  RANGE 0 = grey 0 .. 255, 1 = limited-range video grey 16 .. 235; LO and HI are the disparities x_right - x_left
of the darkest and the brightest grey; DFILTER 1 expands a squeezed depth picture linearly between neighbours at most DGATE (0 .. 255)
codes apart and replicates across larger steps, DFILTER 0 always replicates.  FILL and GATE as --depth-input's.  Nothing is converted
or resampled on the CPU and nothing is matched; excludes --depth-input, --match, --align, --balance, --rectify and the frame bits other
than --linear-warp.
--rectify FILE.npy [BORDER] (an addition; put it behind the positional arguments): both eyes of every frame are first remapped on the
GPU through their rectification records (stm_stream_rectify): FILE.npy is a (2, 18) float32 array, the left eye's record and then the
right eye's (stm_amd.rectify.record makes one from a camera matrix, distortion coefficients, the rectifying rotation and the new
camera matrix).  BORDER 0 (the default): source positions outside an eye read 0; 1: they are clamped.  Everything else then runs on the
rectified pair.  A malformed file is refused before any frame is read; excludes --depth-input.
The angle is truncated to an integer as the reference does (adcensus_stm declares `int angle`, d_io.h:36, and video_io.cpp:158
passes it a float); set STM_EXACT_ANGLE=1 to keep the fractional slant."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv):
    stages = 3 | (0x400 if "--interp" in argv else 0) | (0x200 if "--subpixel" in argv else 0)
    stages |= 0x800 if "--linear-warp" in argv else 0
    stages |= 0x2000 if "--temporal" in argv else 0
    argv = [x for x in argv if x not in ("--interp", "--subpixel", "--linear-warp", "--temporal")]
    temporal = [0.5, 24, 1.5]
    for slot, (flag, conv) in enumerate((("--temporal-alpha", float), ("--temporal-color", int), ("--temporal-disp", float))):
        if flag in argv:
            at = argv.index(flag)
            if at + 1 >= len(argv) or not (stages & 0x2000):
                print(__doc__)
                return -1
            temporal[slot] = conv(argv[at + 1])
            del argv[at:at + 2]
    nv12, matrix = None, 0
    if "--nv12" in argv:
        at = argv.index("--nv12")
        if at + 2 >= len(argv):
            print(__doc__)
            return -1
        nv12 = (int(argv[at + 1]), int(argv[at + 2]))
        del argv[at:at + 3]
    if "--matrix" in argv:
        at = argv.index("--matrix")
        if at + 1 >= len(argv) or nv12 is None:
            print(__doc__)
            return -1
        matrix = int(argv[at + 1])
        del argv[at:at + 2]
    lens = None
    if "--lens" in argv:
        at = argv.index("--lens")
        if at + 4 >= len(argv):
            print(__doc__)
            return -1
        lens = (int(argv[at + 1]), float(argv[at + 2]), float(argv[at + 3]), float(argv[at + 4]))
        del argv[at:at + 5]
    quilt = None
    if "--quilt" in argv:
        at = argv.index("--quilt")
        try:
            quilt = tuple(int(x) for x in argv[at + 1:at + 5])
        except ValueError:
            quilt = ()
        if len(quilt) != 4 or quilt[0] < 1 or quilt[1] < 1 or not 0 <= quilt[2] <= 3 or quilt[3] not in (0, 1) or lens is not None:
            print(__doc__)
            return -1
        del argv[at:at + 5]
    nv12_out = None
    if "--nv12-out" in argv:
        at = argv.index("--nv12-out")
        try:
            nv12_out = int(argv[at + 1])
        except (ValueError, IndexError):
            nv12_out = -1
        if quilt is None or not 0 <= nv12_out <= 3:
            print(__doc__)
            return -1
        del argv[at:at + 2]
    packing = None
    if "--packing" in argv:
        at = argv.index("--packing")
        try:
            packing = tuple(int(x) for x in argv[at + 1:at + 5])
        except ValueError:
            packing = ()
        if len(packing) != 4:
            print(__doc__)
            return -1
        del argv[at:at + 5]
    match = None
    if "--match" in argv:
        at = argv.index("--match")
        try:
            match = (int(argv[at + 1]), int(argv[at + 2]), float(argv[at + 3]))
        except (ValueError, IndexError):
            match = None
        if match is None or match[0] < 1 or match[1] < 1 or not match[2] > 0.0 or packing is not None:
            print(__doc__)
            return -1
        del argv[at:at + 4]
    if "--guided-up" in argv:
        if match is None:
            print(__doc__)
            return -1
        stages |= 0x1000
        argv.remove("--guided-up")
    overlay = None
    if "--overlay" in argv:
        at = argv.index("--overlay")
        try:
            import numpy as np
            pix = np.load(argv[at + 1])
            overlay = (pix, int(argv[at + 2]), int(argv[at + 3]), float(argv[at + 4]))
            if pix.dtype != np.uint8 or pix.ndim != 3 or pix.shape[2] != 4 or 0 in pix.shape or max(pix.shape[:2]) > 65535:
                raise ValueError(pix.shape)
            if max(abs(overlay[1]), abs(overlay[2])) > 65536 or not abs(overlay[3]) <= 4096.0 or nv12_out is not None:
                raise ValueError(overlay[1:])
        except (ValueError, IndexError, OSError):
            print(__doc__)
            return -1
        del argv[at:at + 5]
    overlay_auto = None
    if "--overlay-auto" in argv:
        at = argv.index("--overlay-auto")
        try:
            vals = []
            for x in argv[at + 1:at + 8]:  # LO HI, then up to five optional numbers
                try:
                    vals.append(float(x))
                except ValueError:
                    break
            if len(vals) not in (2, 7) or overlay is None:
                raise ValueError(vals)
            lo, hi = vals[0], vals[1]
            near, margin, pad, rate_near, rate_far = vals[2:] if len(vals) == 7 else (20.0, 1.0, 8.0, 1.0, 0.1)
            if not (lo <= hi and abs(lo) <= 4096.0 and abs(hi) <= 4096.0 and near == int(near) and 0 <= near <= 499 and abs(margin) <= 4096.0
                    and pad == int(pad) and 0 <= pad <= 4096 and 0.0 < rate_near <= 1.0 and 0.0 < rate_far <= 1.0):
                raise ValueError(vals)
            overlay_auto = (lo, hi, int(near), margin, int(pad), rate_near, rate_far)
        except (ValueError, IndexError):
            print(__doc__)
            return -1
        del argv[at:at + 1 + len(vals)]
    depth, depth_auto = None, None
    try:
        if "--depth" in argv:
            at = argv.index("--depth")
            depth = (float(argv[at + 1]), float(argv[at + 2]))
            if not (0.0 <= depth[0] <= 8.0 and abs(depth[1]) <= 4096.0):
                raise ValueError(depth)
            del argv[at:at + 3]
        if "--depth-auto" in argv:
            at = argv.index("--depth-auto")
            vals = []
            for x in argv[at + 1:at + 6]:  # LO HI, then up to three optional numbers
                try:
                    vals.append(float(x))
                except ValueError:
                    break
            if len(vals) not in (2, 5):
                raise ValueError(vals)
            lo, hi = vals[0], vals[1]
            mg, clip, rate = vals[2:] if len(vals) == 5 else (1.0, 20.0, 1.0)
            if not (lo < hi and abs(lo) <= 4096.0 and abs(hi) <= 4096.0 and 0.0 < mg <= 8.0 and clip == int(clip) and 0 <= clip <= 499
                    and 0.0 < rate <= 1.0):
                raise ValueError(vals)
            depth_auto = (lo, hi, mg, int(clip), rate)
            del argv[at:at + 1 + len(vals)]
        if depth is not None and depth_auto is not None:
            raise ValueError("--depth and --depth-auto")
    except (ValueError, IndexError):
        print(__doc__)
        return -1
    antialias = None
    if "--antialias" in argv:
        at = argv.index("--antialias")
        try:
            antialias = (float(argv[at + 1]), int(argv[at + 2]), float(argv[at + 3]))
            if not (0.0 <= antialias[0] <= 8.0 and 1 <= antialias[1] <= 16 and 0.0 <= antialias[2] < float("inf")):
                raise ValueError(antialias)
        except (ValueError, IndexError):
            print(__doc__)
            return -1
        del argv[at:at + 4]
    align, align_auto = None, None
    try:
        if "--align" in argv:
            at = argv.index("--align")
            align = (float(argv[at + 1]), float(argv[at + 2]), float(argv[at + 3]))
            if not all(abs(v) < float("inf") for v in align):
                raise ValueError(align)
            del argv[at:at + 4]
        if "--align-auto" in argv:
            at = argv.index("--align-auto")
            vals = [argv[at + 1]]
            if at + 2 < len(argv) and not argv[at + 2].startswith("--"):
                try:
                    float(argv[at + 2])
                    vals.append(argv[at + 2])
                except ValueError:
                    pass
            align_auto = (int(vals[0]),) + tuple(float(v) for v in vals[1:])
            if not 1 <= align_auto[0] <= 32 or (len(align_auto) > 1 and not 0.0 < align_auto[1] <= 1.0):
                raise ValueError(align_auto)
            del argv[at:at + 1 + len(vals)]
        if align is not None and align_auto is not None:
            raise ValueError("--align and --align-auto")
    except (ValueError, IndexError):
        print(__doc__)
        return -1
    try:
        import stm_amd  # noqa: F401
        from stm_amd import video
        balance, balance_auto = video.take_balance_options(argv)
        cut = video.take_cut_option(argv)
        active, active_auto, active_fill = video.take_active_options(argv)
        maps = video.take_maps_option(argv)
        depth_input = video.take_depth_input_option(argv, stack=True)
        if depth_input is not None and (nv12 is not None or packing is not None or match is not None or align is not None or align_auto is not None
                                        or balance is not None or balance_auto is not None or (stages & ~0x800) != 3):
            raise ValueError("--depth-input")
        rectify = video.take_rectify_option(argv)
        if rectify is not None and depth_input is not None:
            raise ValueError("--rectify")
        depth_video = video.take_depth_video_option(argv)
        if depth_video is not None:
            if (depth_input is not None or rectify is not None or match is not None or align is not None or align_auto is not None
                    or balance is not None or balance_auto is not None or (stages & ~0x800) != 3):
                raise ValueError("--depth-video")
            pk = packing if packing is not None else (0, 0, 0, 0)
            if depth_video[1] and not pk[0] & 1:  # a full-size depth picture is not expanded
                raise ValueError("--depth-video DFILTER")
            depth_video = ("bgr" if nv12 is None else "nv12", matrix) + pk + depth_video
    except (ValueError, IndexError):
        print(__doc__)
        return -1
    if len(argv) not in (16, 17):
        print(__doc__)
        return -1
    import stm_amd  # noqa: F401
    from stm_amd import bmp_io, device_api as dev, video
    a = argv[1:]
    angle = float(a[2]) if os.environ.get("STM_EXACT_ANGLE") == "1" else float(int(float(a[2])))  # SURVEY A-Q24
    p = dev.FrameParams(num_views=int(a[1]), angle=angle, num_disp=int(a[5]), zero_disp=int(a[6]), ad_coeff=float(a[7]),
                        census_coeff=float(a[8]), ucd=float(a[9]), lcd=float(a[10]), usd=int(a[11]), lsd=int(a[12]),
                        thresh_s=int(a[13]), thresh_h=float(a[14]))
    out_w, out_h = int(a[3]), int(a[4])
    out_dir = a[15] if len(a) > 15 else os.path.join(a[0] if nv12 is None else os.path.dirname(os.path.abspath(a[0])), "out")
    frames = video.read_bmp_sequence(a[0]) if nv12 is None else video.read_nv12_sequence(a[0], *nv12)
    if depth_input is not None:  # one image a frame and its plane of the stack
        frames = zip(frames, depth_input[0])
    yuv = None
    if nv12_out is not None:
        os.makedirs(out_dir, exist_ok=True)
        yuv = open(os.path.join(out_dir, "quilt.yuv"), "wb")
    planes = None
    if maps is not None and maps[0] in ("u8", "u16"):
        os.makedirs(out_dir, exist_ok=True)
        planes = open(maps[4] if maps[4] is not None else os.path.join(out_dir, "maps_%s.raw" % maps[0]), "ab")
    cuts = []

    def on_cut(k, c):
        print("frame %d: cut %d score %d since %d" % ((k,) + c))
        if c[0]:
            cuts.append(k)

    t0 = time.perf_counter()
    n = 0
    for (k, dl, dr, inter) in video.process_sequence(frames, p, out_h, out_w, stages, tuple(temporal) if stages & 0x2000 else None,
                                                       "bgr" if nv12 is None or depth_video is not None else "nv12", matrix, lens, depth, depth_auto,
                                                       (lambda k, gc: print("frame %d: gain %.6g conv %.6g" % (k, gc[0], gc[1])))
                                                       if depth_auto is not None else None, packing if depth_video is None else None,
                                                       layout=None if quilt is None else (1,) + quilt, match=match,
                                                       output=None if nv12_out is None else (1, nv12_out), overlay=overlay,
                                                       antialias=antialias, align=align, align_auto=align_auto,
                                                       on_align=(lambda k, f: print("frame %d: align a %.6g b %.6g c %.6g" % ((k,) + f)))
                                                       if align_auto is not None else None,
                                                       balance=balance, balance_auto=balance_auto,
                                                       on_balance=(lambda k, t: print("frame %d: balance B %d %d %d G %d %d %d R %d %d %d" % (
                                                           (k,) + tuple(int(t[c, v]) for c in range(3) for v in (64, 128, 192)))))
                                                       if balance_auto is not None else None,
                                                       cut=cut, on_cut=on_cut if cut is not None else None, overlay_auto=overlay_auto,
                                                       on_overlay_depth=(lambda k, st: print("frame %d: overlay disparity %.6g nearest %.6g" % (
                                                           k, min(max(float(st[1]), overlay_auto[0]), overlay_auto[1]), float(st[2]))))
                                                       if overlay_auto is not None else None,
                                                       active=active, active_auto=active_auto, active_fill=active_fill,
                                                       on_active=(lambda k, r: print("frame %d: active rows %d..%d cols %d..%d changed %d" % ((k,) + r)))
                                                       if active_auto is not None else None,
                                                       maps=None if maps is None else maps[:4],
                                                       depth_input=None if depth_input is None else depth_input[1], rectify=rectify,
                                                       depth_video=depth_video):
        if yuv is not None:  # the frame is [out height * 3 / 2][out width]: the Y plane, then the interleaved UV plane
            yuv.write(inter.tobytes())
        else:
            os.makedirs(out_dir, exist_ok=True)
            bmp_io.write_bmp(os.path.join(out_dir, "interlaced_%05d.bmp" % k), inter)
        if planes is not None:  # the frame's planes, raw and tight: the left one, then the right one, whichever the stream produces
            for plane in (dl, dr):
                if plane is not None:
                    planes.write(plane.tobytes())
        elif dl is not None:
            video.write_disparities(out_dir, k, dl, dr)
        n += 1
    if yuv is not None:
        yuv.close()
    if planes is not None:
        planes.close()
    if cut is not None:
        print("cuts at frames: %s" % " ".join(str(k) for k in cuts))
    dt = time.perf_counter() - t0
    print("%d frames in %.3f s (%.1f frames/s including BMP I/O)" % (n, dt, n / dt if dt > 0 else 0.0))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
