#!/usr/bin/env python
"""Headless counterpart of the reference's still-image driver (image_io.cpp): same 16 positional parameters
(image_io.cpp:118-131), the same per-stage call sequence through the host-flavour API (image_io.cpp:171-292:
IRV x1, bilateral 7/7/7, host-flavour dibr_dbm), BMP files instead of the OpenCV viewer (image_io.cpp:384-469 shows:
source, cost slice, aggregated slice, disparity, outliers, occlusion mask, every view, interlaced output).

usage: stm_image.py <left.bmp> <right.bmp> <ad coeff> <census coeff> <ndisp> <zerodisp> <ucd> <lcd> <usd> <lsd>
                    <num views> <angle> <out width> <out height> <thresh_s> <thresh_h> [out dir] [--interp] [--subpixel]
                    [--linear-warp] [--lens MODE PITCH SLOPE CENTRE] [--quilt TX TY ORDER FILTER]
                    [--antialias STRENGTH MAX_RADIUS GATE] [--align A B C | --align-auto RADIUS [RATE]]
                    [--balance FILE.npy | --balance-auto [MAX_SHIFT RATE]]
                    [--active T B L R | --active-auto [THRESH LIT MAX_BAR HOLD]] [--active-fill DISP]
                    [--depth-input PLANE.npy LO HI [FILL GATE]]
                    [--rectify FILE.npy [BORDER]]
                    [--depth-video RANGE DFILTER DGATE LO HI [FILL GATE] [--packing P SWAP FILTER GAP]]

--interp (an addition, off by default): the outlier interpolation (host_api.dr_interp) of both maps after region voting, each on
its own image and outlier map, before --subpixel.
--subpixel (an addition, off by default): the sub-pixel enhancement (host_api.dc_subpixel) of both maps on their aggregated
volumes after region voting, before the bilateral filter.
--linear-warp (an addition, off by default): every view through host_api.dibr_dbm_lin (both warps fetched at the fractional
coordinate) instead of dibr_dbm.
--lens MODE PITCH SLOPE CENTRE (an addition): the views interlaced through the panel's calibration (host_api.mux_multiview_lens:
PITCH sub-pixels per lens, SLOPE sub-pixels of lens shift per output row, CENTRE lenses of phase offset; MODE 1 = nearest view,
2 = two views blended) instead of the reference's interlacer; <angle> is then ignored.  Mode 3 renders without views: it exists
in the frame calls only (stm_video.py).
--quilt TX TY ORDER FILTER (an addition): the views tiled whole into the output frame (host_api.quilt_multiview: <num views> = TX *
TY tiles; ORDER bit 0 = tile rows bottom-up, bit 1 = tile 0 holds the leftmost camera; FILTER 0 = the reference's four-neighbour
sampler, 1 = the area average) instead of interlaced; <angle> is then ignored.  Excludes --lens.
--antialias STRENGTH MAX_RADIUS GATE (an addition): view antialiasing (host_api.view_prefilter) -- before the views are rendered each
image is blurred along its rows by its own final map: a box of 1 + STRENGTH * |disparity| / (<num views> - 1) pixels (STRENGTH in
[0, 8]), at most MAX_RADIUS (1 .. 16) pixels to a side, using only neighbours whose disparity lies within GATE (>= 0) of the pixel's.
--align A B C (an addition): the right image is first sampled at row y + A + B u + C v (host_api.align_rows; u, v from the image's
centre), so that a vertical offset between the two cameras does not reach the row-wise matcher.  --align-auto RADIUS [RATE]: the
field is measured within +-RADIUS rows (host_api.align_fit) and printed.  The aligned right image is what every later stage sees.
--balance FILE.npy (an addition): the right image then goes through the three tables of FILE.npy (768 bytes of uint8: B, G, R, 256
each; host_api.balance_apply), so that an exposure or white-balance difference between the two cameras reaches neither the matcher
nor the views.  --balance-auto [MAX_SHIFT RATE]: the tables are fitted from the two images' histograms (host_api.balance_fit),
moving no level by more than MAX_SHIFT (48); one still pair: RATE has nothing to follow and is accepted for symmetry.
--active T B L R (an addition): the picture's rectangle inside a letterboxed or pillarboxed pair, rows [T, B) and columns [L, R).
--active-auto [THRESH LIT MAX_BAR HOLD]: the rectangle is measured on the left image (host_api.active_detect: a line is picture
when more than LIT permille (10) of its pixels have a luma above THRESH (24), a bar is at most MAX_BAR permille (300) of the frame to
a side; one still pair: HOLD has nothing to wait for and is accepted for symmetry) and printed.  --active-fill DISP (with either):
both final maps take DISP in the bars (host_api.active_fill) before the views are rendered from them.
--depth-input PLANE.npy LO HI [FILL GATE] (an addition): <left.bmp> comes with its depth plane instead of a right image -- PLANE.npy
holds [H][W] float32, uint8 or uint16 disparities x_right - x_left (the format follows the dtype; code 0 at LO, the largest code at
HI; float32: clamped to the two), <right.bmp> is not read ("-" will do) and the matching parameters are read and ignored.  The second
eye is synthesised on the GPU (stm_stream_input_depth; FILL 0 = the background extended into the holes, 1 = continued from the mirror
pixel within GATE) and the frame rendered by a one-frame stream, which has no per-stage products: disp_l (the decoded plane), disp_r
(the synthesised map) and the output frame are written.  Excludes --interp, --subpixel, --align, --balance and their -auto forms.
--rectify FILE.npy [BORDER] (an addition; put it behind the positional arguments): both images are first remapped on the GPU through
their rectification records (host_api.rectify): FILE.npy is a (2, 18) float32 array, the left eye's record and then the right eye's
(stm_amd.rectify.record).  BORDER 0 (the default): source positions outside an image read 0; 1: they are clamped.  Every stage then
runs on the rectified pair.  A malformed file is refused before any image is read; excludes --depth-input.
--depth-video RANGE DFILTER DGATE LO HI [FILL GATE] (an addition): <left.bmp> is one packed 2D-plus-depth frame, the image in one half
and its depth as a grey picture in the other (stm_stream_input_packed_depth); --packing P SWAP FILTER GAP (stm_set_packing's
settings; only with this option; without it: side by side, full size) says where the halves lie.  RANGE 0 = grey 0 .. 255, 1 = 16 ..
235; LO and HI are the disparities of the darkest and the brightest grey; DFILTER 1 expands a squeezed depth picture linearly between
neighbours at most DGATE codes apart.  <right.bmp> is not read and one frame goes through a stream, as with --depth-input, which it
excludes together with what that option excludes and --rectify."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def depth_input_frame(a, depth_input, linear_warp, lens, quilt, antialias, active, active_auto, active_fill, depth_video=None):
    """--depth-input: the left image and its plane through a one-frame stream; --depth-video: the packed frame likewise"""
    import stm_amd
    from stm_amd import device_api as dev, video
    L = stm_amd.bmp_io.read_bmp(a[0])
    if depth_video is not None:
        plane, setting = None, None
        H, W = video.unpacked_eye_shape(L.shape[0], L.shape[1], depth_video[2:6])
    else:
        plane, setting = depth_input
        H, W = L.shape[:2]
    if plane is not None and plane.shape != L.shape[:2]:
        print("Error! the image is %d x %d, the depth plane %s" % (L.shape[0], L.shape[1], plane.shape))
        return -1
    N, angle, Wo, Ho = int(a[10]), float(a[11]), int(a[12]), int(a[13])
    out = a[16] if len(a) > 16 else "stm_out"
    os.makedirs(out, exist_ok=True)
    try:
        fs = video.FrameStream(H, W, dev.FrameParams(num_views=N, angle=angle), Ho, Wo, 3 | (0x800 if linear_warp else 0),
                               lens=lens, layout=None if quilt is None else (1,) + quilt, antialias=antialias, active=active,
                               active_auto=active_auto, active_fill=active_fill, depth_input=setting, depth_video=depth_video,
                               depth_pitch=None if depth_video is None else L.shape[1])
    except ValueError as e:
        print("Error! %s" % e)
        return -1
    try:
        if depth_video is not None:
            fs.submit(L)
        else:
            fs.submit_depth(L, plane)
        _, dl, dr, frame = fs.collect()
    finally:
        fs.close()
    for name, img in (("disp_l", video.normalize_minmax_u8(dl)), ("disp_r", video.normalize_minmax_u8(dr)), ("interlaced", frame)):
        stm_amd.bmp_io.write_bmp(os.path.join(out, name + ".bmp"), img)
    print("wrote 3 files to %s (%dx%d, %d views, depth input %s)" % (out, W, H, N, "packed video" if setting is None else setting[0]))
    return 0


def main(argv):
    subpixel, interp, linear_warp = "--subpixel" in argv, "--interp" in argv, "--linear-warp" in argv
    argv = [x for x in argv if x not in ("--subpixel", "--interp", "--linear-warp")]
    quilt = None
    if "--quilt" in argv:
        at = argv.index("--quilt")
        try:
            quilt = tuple(int(x) for x in argv[at + 1:at + 5])
        except ValueError:
            quilt = ()
        if len(quilt) != 4 or quilt[0] < 1 or quilt[1] < 1 or not 0 <= quilt[2] <= 3 or quilt[3] not in (0, 1) or "--lens" in argv:
            print(__doc__)
            return -1
        del argv[at:at + 5]
    lens = None
    if "--lens" in argv:
        at = argv.index("--lens")
        if at + 4 >= len(argv) or argv[at + 1] not in ("1", "2"):
            print(__doc__)
            return -1
        lens = (int(argv[at + 1]), float(argv[at + 2]), float(argv[at + 3]), float(argv[at + 4]))
        del argv[at:at + 5]
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
        if "--align-auto" in argv:  # one still pair: RATE has nothing to follow and is accepted for symmetry
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
        active, active_auto, active_fill = video.take_active_options(argv)
        depth_input = video.take_depth_input_option(argv)
        if depth_input is not None and (subpixel or interp or align is not None or align_auto is not None or balance is not None
                                        or balance_auto is not None):
            raise ValueError("--depth-input")
        rectify = video.take_rectify_option(argv)
        if rectify is not None and depth_input is not None:
            raise ValueError("--rectify")
        depth_video = video.take_depth_video_option(argv)
        packing = None
        if "--packing" in argv:
            at = argv.index("--packing")
            packing = tuple(int(x) for x in argv[at + 1:at + 5])
            if len(packing) != 4 or depth_video is None:
                raise ValueError("--packing")
            del argv[at:at + 5]
        if depth_video is not None:
            if (depth_input is not None or rectify is not None or subpixel or interp or align is not None or align_auto is not None
                    or balance is not None or balance_auto is not None):
                raise ValueError("--depth-video")
            pk = packing if packing is not None else (0, 0, 0, 0)
            if depth_video[1] and not pk[0] & 1:  # a full-size depth picture is not expanded
                raise ValueError("--depth-video DFILTER")
            depth_video = ("bgr", 0) + pk + depth_video
    except (ValueError, IndexError):
        print(__doc__)
        return -1
    if len(argv) not in (17, 18):
        print(__doc__)
        return -1
    import stm_amd
    from stm_amd import host_api as api, video
    a = argv[1:]
    if depth_input is not None or depth_video is not None:
        return depth_input_frame(a, depth_input, linear_warp, lens, quilt, antialias, active, active_auto, active_fill, depth_video)
    L, R = stm_amd.bmp_io.read_bmp(a[0]), stm_amd.bmp_io.read_bmp(a[1])
    if L.shape != R.shape:
        print("Error! left and right image sizes differ: %s vs %s" % (L.shape, R.shape))
        return -1
    if rectify is not None:  # first of all: everything below runs on the rectified pair
        L, R = api.rectify(L, rectify[0], rectify[2]), api.rectify(R, rectify[1], rectify[2])
    if align_auto is not None:
        st, nvalid = api.align_fit(L, R, align_auto[0])
        align = tuple(float(v) for v in st[1:])
        print("align: a %.6g b %.6g c %.6g (%d of 32 blocks)" % (align + (nvalid,)))
    if align is not None:
        R = api.align_rows(R, *align)
    if balance_auto is not None:
        balance = api.balance_lut(api.balance_fit(L, R, balance_auto[0]))
        print("balance: B %d %d %d G %d %d %d R %d %d %d" % tuple(int(balance[c, v]) for c in range(3) for v in (64, 128, 192)))
    if balance is not None:
        R = api.balance_apply(R, balance)
    if active_auto is not None:  # on the left image as given: the reference of the alignment and the balance
        active = tuple(int(v) for v in api.active_detect(L, *active_auto[:3], hold=1, restart=True)[1][1:5])
        print("active: rows %d..%d cols %d..%d" % active)
    if active is not None and not (active[1] <= L.shape[0] and active[3] <= L.shape[1]):
        print("Error! --active %d %d %d %d does not fit a %d x %d image" % (active + L.shape[:2]))
        return -1
    ad, ce, D, zd = float(a[2]), float(a[3]), int(a[4]), int(a[5])
    ucd, lcd, usd, lsd = float(a[6]), float(a[7]), int(a[8]), int(a[9])
    N, angle, Wo, Ho, ts, th = int(a[10]), float(a[11]), int(a[12]), int(a[13]), int(a[14]), float(a[15])
    out = a[16] if len(a) > 16 else "stm_out"
    os.makedirs(out, exist_ok=True)
    H, W, _ = L.shape
    wr = lambda name, img: stm_amd.bmp_io.write_bmp(os.path.join(out, name + ".bmp"), img)
    cl, cr = api.ci_adcensus(L, R, ad, ce, D, zd)                         # image_io.cpp:171
    xl, al = api.ca_cross(L, cl, ucd, lcd, usd, lsd)                      # :209
    xr, ar = api.ca_cross(R, cr, ucd, lcd, usd, lsd)                      # :210
    dl, dr = api.dc_wta(al, zd), api.dc_wta(ar, zd)                       # :222-223
    wr("cost_l_zd", video.normalize_minmax_u8(cl[min(max(zd, 0), D - 1)]))
    wr("acost_l_zd", video.normalize_minmax_u8(al[min(max(zd, 0), D - 1)]))
    wr("disp_wta_l", video.normalize_minmax_u8(dl))
    ol, orr = api.dr_dcc(dl, dr)                                          # :235
    dl, ol = api.dr_irv(dl, ol, xl, ts, th, D, zd, usd, 1)                # :237
    dr, orr = api.dr_irv(dr, orr, xr, ts, th, D, zd, usd, 1)              # :238
    if interp:
        dl, dr = api.dr_interp(dl, ol, L), api.dr_interp(dr, orr, R)
    if subpixel:
        dl, dr = api.dc_subpixel(al, dl, zd), api.dc_subpixel(ar, dr, zd)
    dl = api.filter_bilateral_1(dl, 7, 7.0, 7.0, D)                       # :242
    dr = api.filter_bilateral_1(dr, 7, 7.0, 7.0, D)                       # :243
    if active is not None and active_fill is not None:
        dl, dr = api.active_fill(dl, active, active_fill), api.active_fill(dr, active, active_fill)
    wr("disp_l", video.normalize_minmax_u8(dl)); wr("disp_r", video.normalize_minmax_u8(dr))
    wr("outliers_l", (ol.astype(np.uint16) * 127).astype(np.uint8)); wr("outliers_r", (orr.astype(np.uint16) * 127).astype(np.uint8))
    occl_l, occl_r = api.dibr_occl(dl, dr)                                # :255
    occl_l, occl_r = api.filter_bleed_1(occl_l, 1), api.filter_bleed_1(occl_r, 1)   # :257-258
    ml, mr = api.dibr_occl_to_mask(occl_l, occl_r)                        # :266
    wr("mask_l", (ml * 255).astype(np.uint8)); wr("mask_r", (mr * 255).astype(np.uint8))
    dbm = api.dibr_dbm_lin if linear_warp else api.dibr_dbm
    if antialias is not None:  # every view, the two end views included, from the prefiltered pair
        L, R = api.view_prefilter(L, dl, N, *antialias), api.view_prefilter(R, dr, N, *antialias)
    views = [R]                                                          # :268-272: views[0] = right, views[N-1] = left
    for v in range(1, N - 1):
        shift = float(np.float32(1.0 - (1.0 * np.float32(v)) / (np.float32(N) - 1.0)))   # :281
        views.append(dbm(L, R, dl, dr, occl_l, occl_r, ml, mr, shift))                    # :282
    views.append(L)
    for v, img in enumerate(views):
        wr("view_%d" % v, img)
    if quilt is not None:
        wr("interlaced", api.quilt_multiview(views, *quilt, Ho, Wo))
    else:
        wr("interlaced", api.mux_multiview(views, angle, Ho, Wo) if lens is None else api.mux_multiview_lens(views, *lens, Ho, Wo))  # :292
    print("wrote %d files to %s (%dx%d, D=%d, %d views)" % (len(os.listdir(out)), out, W, H, D, N))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
