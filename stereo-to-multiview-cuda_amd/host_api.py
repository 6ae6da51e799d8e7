"""Host-flavour stage API: numpy in, numpy out, every call crosses host<->device like the reference's
`stage(host ptrs...)` wrappers that image_io.cpp:171-292 calls.  Names, argument order and semantics follow
the reference headers (d_*.h); the arrays replace the raw pointers:

  images       uint8  [H][W][3]  BGR
  cost volume  float32 [D][H][W] (the C ABI receives it as the reference's table of D plane pointers)
  cross arms   uint8  [4][H][W]  UP, DOWN, LEFT, RIGHT
  disparity    float32 [H][W]
All work happens in libstm_hip.so (HIP kernels); nothing here computes.
"""
import ctypes as C

import numpy as np

from ._lib import f32p, f32pp, lib, u32p, u8p, u8pp


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a, a.ctypes.data_as(u8p)


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(f32p)


def _plane_table_f32(vol):
    """float** over the planes of a contiguous [D][H][W] array."""
    D = vol.shape[0]
    return (f32p * D)(*[vol[d].ctypes.data_as(f32p) for d in range(D)])


def _plane_table_u8(vol):
    n = vol.shape[0]
    return (u8p * n)(*[vol[k].ctypes.data_as(u8p) for k in range(n)])


def ci_adcensus(img_l, img_r, ad_coeff, census_coeff, num_disp, zero_disp):
    """d_ci_adcensus.h:23-25.  Returns (cost_l, cost_r), each [D][H][W]."""
    H, W, E = img_l.shape
    img_l, pl = _u8(img_l)
    img_r, pr = _u8(img_r)
    cl = np.zeros((num_disp, H, W), np.float32)
    cr = np.zeros((num_disp, H, W), np.float32)
    lib().stm_ci_adcensus(pl, pr, C.cast(_plane_table_f32(cl), f32pp), C.cast(_plane_table_f32(cr), f32pp),
                          ad_coeff, census_coeff, num_disp, zero_disp, H, W, E)
    return cl, cr


def ca_cross(img, cost, ucd, lcd, usd, lsd):
    """d_ca_cross.h:19-21.  Returns (cross[4][H][W], acost[D][H][W]); `cost` is left untouched."""
    H, W, E = img.shape
    img, pi = _u8(img)
    cost, _ = _f32(cost)
    D = cost.shape[0]
    cross = np.zeros((4, H, W), np.uint8)
    acost = np.zeros_like(cost)
    lib().stm_ca_cross(pi, C.cast(_plane_table_u8(cross), u8pp), C.cast(_plane_table_f32(cost), f32pp),
                       C.cast(_plane_table_f32(acost), f32pp), ucd, lcd, usd, lsd, D, H, W, E)
    return cross, acost


def dc_wta(cost, zero_disp):
    """d_dc_wta.h:16-18."""
    cost, _ = _f32(cost)
    D, H, W = cost.shape
    disp = np.zeros((H, W), np.float32)
    lib().stm_dc_wta(C.cast(_plane_table_f32(cost), f32pp), disp.ctypes.data_as(f32p), D, zero_disp, H, W)
    return disp


def dc_subpixel(cost, disp, zero_disp):
    """Sub-pixel enhancement of `disp` on the aggregated volume `cost` (stm_dc_subpixel; an addition, the reference has no such
    step).  Returns the refined map; `disp` is not modified."""
    cost, _ = _f32(cost)
    D, H, W = cost.shape
    out = np.array(disp, dtype=np.float32, order="C", copy=True)
    assert out.shape == (H, W)
    lib().stm_dc_subpixel(C.cast(_plane_table_f32(cost), f32pp), out.ctypes.data_as(f32p), D, zero_disp, H, W)
    return out


def dc_hslo(cost, img_l, img_r, T, H1, H2, zero_disp):
    """d_dc_hslo.h:18-22 (parity unpinned: the reference is a stub)."""
    cost, _ = _f32(cost)
    D, H, W = cost.shape
    img_l, pl = _u8(img_l)
    img_r, pr = _u8(img_r)
    disp = np.zeros((H, W), np.float32)
    lib().stm_dc_hslo(C.cast(_plane_table_f32(cost), f32pp), disp.ctypes.data_as(f32p), pl, pr, T, H1, H2,
                      D, zero_disp, H, W, img_l.shape[2])
    return disp


def dr_dcc(disp_l, disp_r):
    """d_dr_dcc.h:17-19.  Returns (outliers_l, outliers_r) in {0,1,2}."""
    disp_l, pl = _f32(disp_l)
    disp_r, pr = _f32(disp_r)
    H, W = disp_l.shape
    ol = np.zeros((H, W), np.uint8)
    orr = np.zeros((H, W), np.uint8)
    lib().stm_dr_dcc(ol.ctypes.data_as(u8p), orr.ctypes.data_as(u8p), pl, pr, H, W)
    return ol, orr


def dr_irv(disp, outliers, cross, thresh_s, thresh_h, num_disp, zero_disp, usd, iterations):
    """d_dr_irv.h:15-19 (in place in the reference; copies are returned here)."""
    disp = np.array(disp, dtype=np.float32, order="C", copy=True)
    outliers = np.array(outliers, dtype=np.uint8, order="C", copy=True)
    cross, _ = _u8(cross)
    H, W = disp.shape
    lib().stm_dr_irv(disp.ctypes.data_as(f32p), outliers.ctypes.data_as(u8p), C.cast(_plane_table_u8(cross), u8pp),
                     thresh_s, thresh_h, H, W, num_disp, zero_disp, usd, iterations)
    return disp, outliers


def dr_interp(disp, outliers, img):
    """Outlier interpolation (stm_dr_interp; an addition, the reference has no such step): every pixel with outliers != 0 takes
    the value of a reliable pixel found along 16 directions -- class 2 the largest, any other class the closest in colour in
    `img`, the same view's image.  Returns the refined map; nothing passed in is modified."""
    out = np.array(disp, dtype=np.float32, order="C", copy=True)
    outliers, po = _u8(outliers)
    img, pi = _u8(img)
    H, W = out.shape
    assert outliers.shape == (H, W) and img.shape[:2] == (H, W) and img.ndim == 3
    lib().stm_dr_interp(out.ctypes.data_as(f32p), po, pi, H, W, img.shape[2])
    return out


def filter_bilateral_1(img, radius, sigma_color, sigma_spatial, num_disp):
    """d_filter_bilateral.h:17-20."""
    img = np.array(img, dtype=np.float32, order="C", copy=True)
    H, W = img.shape
    lib().stm_filter_bilateral_1(img.ctypes.data_as(f32p), radius, sigma_color, sigma_spatial, H, W, num_disp)
    return img


def filter_gaussian_1(img, radius, sigma_spatial):
    """d_filter_gaussian.h:20-22 (grow-only: out = max(in, blur))."""
    img = np.array(img, dtype=np.float32, order="C", copy=True)
    H, W = img.shape
    lib().stm_filter_gaussian_1(img.ctypes.data_as(f32p), radius, sigma_spatial, H, W)
    return img


def filter_median(img):
    """d_filter.h:11-12."""
    img = np.array(img, dtype=np.float32, order="C", copy=True)
    H, W = img.shape
    lib().stm_filter_median(img.ctypes.data_as(f32p), H, W)
    return img


def filter_bleed_1(img, radius):
    """d_filter.h:26-28."""
    img = np.array(img, dtype=np.uint8, order="C", copy=True)
    H, W = img.shape
    lib().stm_filter_bleed_1(img.ctypes.data_as(u8p), radius, H, W)
    return img


def dibr_occl(disp_l, disp_r):
    """d_dibr_occl.h:31-33.  Returns (occl_l, occl_r) hit maps."""
    disp_l, pl = _f32(disp_l)
    disp_r, pr = _f32(disp_r)
    H, W = disp_l.shape
    ol = np.zeros((H, W), np.uint8)
    orr = np.zeros((H, W), np.uint8)
    lib().stm_dibr_occl(ol.ctypes.data_as(u8p), orr.ctypes.data_as(u8p), pl, pr, H, W)
    return ol, orr


def dibr_occl_to_mask(occl_l, occl_r):
    """d_dibr_occl.h:18-20."""
    occl_l, pl = _u8(occl_l)
    occl_r, pr = _u8(occl_r)
    H, W = occl_l.shape
    ml = np.zeros((H, W), np.float32)
    mr = np.zeros((H, W), np.float32)
    lib().stm_dibr_occl_to_mask(ml.ctypes.data_as(f32p), mr.ctypes.data_as(f32p), pl, pr, H, W)
    return ml, mr


def dibr_dbm(img_l, img_r, disp_l, disp_r, occl_l, occl_r, mask_l, mask_r, shift):
    """d_dibr_bwarp.h:29-34 (host flavour: mask blur gaussian(7,10))."""
    H, W, E = img_l.shape
    img_l, pil = _u8(img_l)
    img_r, pir = _u8(img_r)
    disp_l, pdl = _f32(disp_l)
    disp_r, pdr = _f32(disp_r)
    occl_l, pol = _u8(occl_l)
    occl_r, por = _u8(occl_r)
    mask_l, pml = _f32(mask_l)
    mask_r, pmr = _f32(mask_r)
    out = np.zeros((H, W, E), np.uint8)
    lib().stm_dibr_dbm(out.ctypes.data_as(u8p), pil, pir, pdl, pdr, pol, por, pml, pmr, shift, H, W, E)
    return out


def dibr_dbm_lin(img_l, img_r, disp_l, disp_r, occl_l, occl_r, mask_l, mask_r, shift):
    """dibr_dbm with both backward warps fetched at the fractional warp coordinate (stm_dibr_dbm_lin; an addition, the reference
    truncates the coordinate).  Host flavour: mask blur gaussian(7,10)."""
    H, W, E = img_l.shape
    img_l, pil = _u8(img_l)
    img_r, pir = _u8(img_r)
    disp_l, pdl = _f32(disp_l)
    disp_r, pdr = _f32(disp_r)
    occl_l, pol = _u8(occl_l)
    occl_r, por = _u8(occl_r)
    mask_l, pml = _f32(mask_l)
    mask_r, pmr = _f32(mask_r)
    out = np.zeros((H, W, E), np.uint8)
    lib().stm_dibr_dbm_lin(out.ctypes.data_as(u8p), pil, pir, pdl, pdr, pol, por, pml, pmr, shift, H, W, E)
    return out


def dibr_dfm(img_l, img_r, disp_l, disp_r, shift):
    """d_dibr_fwarp.h:17-20 (deterministic; parity unpinned)."""
    H, W, E = img_l.shape
    img_l, pil = _u8(img_l)
    img_r, pir = _u8(img_r)
    disp_l, pdl = _f32(disp_l)
    disp_r, pdr = _f32(disp_r)
    out = np.zeros((H, W, E), np.uint8)
    lib().stm_dibr_dfm(out.ctypes.data_as(u8p), pil, pir, pdl, pdr, shift, H, W, E)
    return out


def mux_multiview(views, angle, out_rows, out_cols):
    """d_mux_multiview.h:39-41.  views[0] = right image ... views[N-1] = left image."""
    views = [np.ascontiguousarray(v, dtype=np.uint8) for v in views]
    N = len(views)
    H, W, E = views[0].shape
    tab = (u8p * N)(*[v.ctypes.data_as(u8p) for v in views])
    out = np.zeros((out_rows, out_cols, E), np.uint8)
    lib().stm_mux_multiview(C.cast(tab, u8pp), out.ctypes.data_as(u8p), N, angle, H, W, out_rows, out_cols, E)
    return out


def mux_multiview_lens(views, mode, pitch, slope, centre, out_rows, out_cols):
    """stm_mux_multiview_lens (an addition, the reference's interlacer fits one panel): mux_multiview with each sub-pixel's view
    taken from its phase under a lens sheet of `pitch` sub-pixels per lens, slanted by `slope` sub-pixels per row, offset by
    `centre` lenses; mode 1 = the nearest view, 2 = the two nearest views blended."""
    views = [np.ascontiguousarray(v, dtype=np.uint8) for v in views]
    N = len(views)
    H, W, E = views[0].shape
    tab = (u8p * N)(*[v.ctypes.data_as(u8p) for v in views])
    out = np.zeros((out_rows, out_cols, E), np.uint8)
    lib().stm_mux_multiview_lens(C.cast(tab, u8pp), out.ctypes.data_as(u8p), N, int(mode), float(pitch), float(slope), float(centre),
                                 H, W, out_rows, out_cols, E)
    return out


def quilt_multiview(views, tiles_x, tiles_y, order, filter, out_rows, out_cols):
    """stm_quilt_multiview (an addition): the views tiled into one out_rows x out_cols frame, view v whole in tile k = v (order bit
    1: N - 1 - v) of tiles_x x tiles_y tiles counted row by row from the top (order bit 0: from the bottom); filter 0 = the
    reference's four-neighbour sampler, 1 = the area average.  Pixels outside every tile are 0."""
    views = [np.ascontiguousarray(v, dtype=np.uint8) for v in views]
    N = len(views)
    H, W, E = views[0].shape
    tab = (u8p * N)(*[v.ctypes.data_as(u8p) for v in views])
    out = np.zeros((out_rows, out_cols, E), np.uint8)
    lib().stm_quilt_multiview(C.cast(tab, u8pp), out.ctypes.data_as(u8p), N, int(tiles_x), int(tiles_y), int(order), int(filter),
                              H, W, out_rows, out_cols, E)
    return out


def mux_overlay(frame, overlay, x0, y0, disparity, num_views, angle=18.43, lens=None, layout=None):
    """stm_mux_overlay (an addition): the overlay (uint8 [rows][cols][4], premultiplied B, G, R, A) composited into a copy of the
    finished frame (uint8 [Ho][Wo][E]) at view pixel (x0, y0) -- a pixel of the frame, or of every tile of a quilt -- and at the
    end-to-end `disparity` (> 0 behind the screen, < 0 in front).  lens = (mode, pitch, slope, centre), None = the reference's
    interlacer at `angle`; layout = (1, tiles_x, tiles_y, order) for a quilt, None = the interlaced frame.  Returns the frame."""
    out = np.array(frame, dtype=np.uint8, order="C")
    overlay, po = _u8(overlay)
    assert out.ndim == 3 and overlay.ndim == 3 and overlay.shape[2] == 4
    ln = tuple(lens) if lens is not None else (0, 0.0, 0.0, 0.0)
    lo = tuple(layout)[:4] if layout is not None else (0, 1, 1, 0)
    lib().stm_mux_overlay(out.ctypes.data_as(u8p), po, overlay.shape[0], overlay.shape[1], int(x0), int(y0), float(disparity),
                          int(num_views), float(angle), int(ln[0]), float(ln[1]), float(ln[2]), float(ln[3]), int(lo[0]), int(lo[1]),
                          int(lo[2]), int(lo[3]), out.shape[0], out.shape[1], out.shape[2])
    return out


def _frame_out(out_rows, out_cols, E):
    """the array a rendering frame call fills: the BGR frame, or -- under stm_set_output's format 1 -- the NV12 surface of
    (R + out_rows / 2) x P bytes (P = pitch or out_cols, R = uv_row or out_rows)"""
    now = (C.c_int * 4)()
    lib().stm_get_output(now)
    if now[0] == 0:
        return np.zeros((out_rows, out_cols, E), np.uint8)
    return np.zeros(((now[3] or out_rows) + out_rows // 2, now[2] or out_cols), np.uint8)


def adcensus_stm(img_sbs, num_cols, out_rows, out_cols, num_views, angle, num_disp, zero_disp,
                 ad_coeff, census_coeff, ucd, lcd, usd, lsd, thresh_s, thresh_h):
    """d_io.h:32-40: host SBS frame in, (disp_l, disp_r, interlaced) out (interlaced: the frame, or the NV12 surface of _frame_out)."""
    img_sbs, ps = _u8(img_sbs)
    H, Wsbs, E = img_sbs.shape
    dl = np.zeros((H, num_cols), np.float32)
    dr = np.zeros((H, num_cols), np.float32)
    out = _frame_out(out_rows, out_cols, E)
    lib().stm_adcensus_stm(ps, dl.ctypes.data_as(f32p), dr.ctypes.data_as(f32p), out.ctypes.data_as(u8p),
                           H, Wsbs, num_cols, out_rows, out_cols, E, num_views, angle, num_disp, zero_disp,
                           ad_coeff, census_coeff, ucd, lcd, usd, lsd, thresh_s, thresh_h)
    return dl, dr, out


def adcensus_stm_2(img_sbs, num_cols, out_rows, out_cols, disp_rows, disp_cols, disp_scale, num_views, angle, num_disp,
                   zero_disp, ad_coeff, census_coeff, ucd, lcd, usd, lsd, thresh_s, thresh_h):
    """d_io.h:42-52: disparity at reduced resolution (disp_rows x disp_cols), views at full resolution."""
    img_sbs, ps = _u8(img_sbs)
    H, Wsbs, E = img_sbs.shape
    dl = np.zeros((H, num_cols), np.float32)
    dr = np.zeros((H, num_cols), np.float32)
    out = _frame_out(out_rows, out_cols, E)
    lib().stm_adcensus_stm_2(ps, dl.ctypes.data_as(f32p), dr.ctypes.data_as(f32p), out.ctypes.data_as(u8p),
                             H, Wsbs, num_cols, out_rows, out_cols, disp_rows, disp_cols, E, disp_scale, num_views, angle,
                             num_disp, zero_disp, ad_coeff, census_coeff, ucd, lcd, usd, lsd, thresh_s, thresh_h)
    return dl, dr, out


def adcensus_stm_2s(img_sbs, num_cols, out_rows, out_cols, disp_rows, disp_cols, disp_scale, num_views, angle, num_disp,
                    zero_disp, ad_coeff, census_coeff, ucd, lcd, usd, lsd, thresh_s, thresh_h, stages=3):
    """adcensus_stm_2 with a `stages` word (stm_adcensus_stm_2s): 3, optionally OR-ed with 0x100, 0x200, 0x400 (the match on the
    reduced pair), 0x800 (linear sampling in the render) and 0x1000 (guided up-sampling of the maps).  stages = 3 is adcensus_stm_2."""
    img_sbs, ps = _u8(img_sbs)
    H, Wsbs, E = img_sbs.shape
    dl = np.zeros((H, num_cols), np.float32)
    dr = np.zeros((H, num_cols), np.float32)
    out = _frame_out(out_rows, out_cols, E)
    lib().stm_adcensus_stm_2s(ps, dl.ctypes.data_as(f32p), dr.ctypes.data_as(f32p), out.ctypes.data_as(u8p),
                              H, Wsbs, num_cols, out_rows, out_cols, disp_rows, disp_cols, E, disp_scale, num_views, angle,
                              num_disp, zero_disp, ad_coeff, census_coeff, ucd, lcd, usd, lsd, thresh_s, thresh_h, stages)
    return dl, dr, out


def disp_upsample(disp_low, img_low, img, up, sigma_color=15.0):
    """Guided disparity up-sampling (stm_disp_upsample; an addition, the reference scales its maps up bilinearly): the map
    disp_low [h][w], computed on img_low [h][w][E], brought to the size of the guide image img [H][W][E], every tap weighted by
    its colour similarity to the guide pixel; values multiplied by `up`.  Returns the [H][W] map; nothing passed in is modified."""
    disp_low, pd = _f32(disp_low)
    img_low, pl = _u8(img_low)
    img, pi = _u8(img)
    h, w = disp_low.shape
    H, W, E = img.shape
    assert img_low.shape == (h, w, E)
    out = np.zeros((H, W), np.float32)
    lib().stm_disp_upsample(out.ctypes.data_as(f32p), pd, pl, pi, H, W, h, w, E, float(up), float(sigma_color))
    return out


def disp_temporal(disp, disp_prev, img, img_prev, alpha=0.5, thresh_color=24, thresh_disp=1.5):
    """Temporal disparity stabilisation (stm_disp_temporal; an addition, the reference matches every frame on its own): this
    frame's filtered map disp [H][W] pulled towards disp_prev, the map the previous frame put out, by the weight alpha wherever
    the 3 x 3 maximum of the colour change between img_prev and img [H][W][E] is at most thresh_color and the maps differ by at
    most thresh_disp.  Returns the [H][W] map; nothing passed in is modified."""
    out = np.array(disp, dtype=np.float32, order="C")  # a copy: the library rewrites it in place
    disp_prev, pq = _f32(disp_prev)
    img, pi = _u8(img)
    img_prev, pp = _u8(img_prev)
    H, W, E = img.shape
    assert out.shape == (H, W) and disp_prev.shape == (H, W) and img_prev.shape == img.shape
    lib().stm_disp_temporal(out.ctypes.data_as(f32p), pq, pi, pp, H, W, E, float(alpha), int(thresh_color), float(thresh_disp))
    return out


def depth_fit(disp_l, disp_r, disp_lo, disp_hi, max_gain=1.0, clip_permille=20, rate=1.0, state=None):
    """The measurement of the automatic depth budget (stm_depth_fit; an addition, the reference's views always span the camera
    baseline): the gain and convergence that bring the clipped disparity range of the two maps [H][W] into [disp_lo, disp_hi],
    folded into `state` = (valid, gain, conv, 0) (None = no history).  Returns the new state as a float32 array of four; nothing
    passed in is modified."""
    disp_l, pl = _f32(disp_l)
    disp_r, pr = _f32(disp_r)
    H, W = disp_l.shape
    assert disp_r.shape == (H, W)
    st = np.zeros(4, np.float32) if state is None else np.array(state, dtype=np.float32, order="C")
    assert st.shape == (4,)
    lib().stm_depth_fit(pl, pr, H, W, float(disp_lo), float(disp_hi), float(max_gain), int(clip_permille), float(rate),
                        st.ctypes.data_as(f32p))
    return st


def overlay_fit(disp_l, disp_r, overlay, x0, y0, view_rows, view_cols, limit_lo, limit_hi, gain=1.0, conv=0.0, near_permille=20, margin=1.0,
                pad=8, rate_near=1.0, rate_far=0.1, restart=False, state=None):
    """The measurement of the overlay's automatic depth placement (stm_overlay_fit; an addition, the reference has no overlay): the
    disparity that keeps the overlay [rows][cols][4] at (x0, y0) of the view view_rows x view_cols in front of what the two maps
    [H][W] show under its alpha box, folded into `state` = (valid, disparity, nearest, 0) (None = no history).  Returns the new
    state as a float32 array of four; nothing passed in is modified."""
    disp_l, pl = _f32(disp_l)
    disp_r, pr = _f32(disp_r)
    overlay, po = _u8(overlay)
    H, W = disp_l.shape
    assert disp_r.shape == (H, W) and overlay.ndim == 3 and overlay.shape[2] == 4
    st = np.zeros(4, np.float32) if state is None else np.array(state, dtype=np.float32, order="C")
    assert st.shape == (4,)
    lib().stm_overlay_fit(pl, pr, H, W, po, overlay.shape[0], overlay.shape[1], int(x0), int(y0), int(view_rows), int(view_cols), float(gain),
                          float(conv), int(near_permille), float(margin), int(pad), float(limit_lo), float(limit_hi), float(rate_near),
                          float(rate_far), int(bool(restart)), st.ctypes.data_as(f32p))
    return st


def view_prefilter(img, disp, num_views, strength=1.0, max_radius=8, gate=1.0, gain=1.0, conv=0.0):
    """View antialiasing (stm_view_prefilter; an addition, the reference's views are pinhole images): img [H][W][E] filtered along
    its rows by its own map disp [H][W] -- a box of 1 + strength * |gain * disp - conv| / (num_views - 1) pixels, at most max_radius
    to a side, whose taps are used only where the map stays within `gate` of the pixel's own value.  Returns the [H][W][E] image
    (bytes of a pixel past the third are 0); nothing passed in is modified."""
    img, pi = _u8(img)
    disp, pd = _f32(disp)
    H, W, E = img.shape
    assert disp.shape == (H, W)
    out = np.zeros((H, W, E), np.uint8)
    lib().stm_view_prefilter(out.ctypes.data_as(u8p), pi, pd, H, W, E, int(num_views), float(strength), int(max_radius), float(gate),
                             float(gain), float(conv))
    return out


def align_rows(img, a, b, c):
    """The vertical alignment applied to one image (stm_align_rows; an addition, the reference takes rectified pairs): img
    [H][W][E] sampled at row y + a + b u + c v (u, v from the image's centre), two rows blended in sixteenths, rows clamped to the
    image.  Returns the [H][W][E] image (bytes of a pixel past the third are 0); nothing passed in is modified."""
    img, pi = _u8(img)
    H, W, E = img.shape
    out = np.zeros((H, W, E), np.uint8)
    lib().stm_align_rows(out.ctypes.data_as(u8p), pi, H, W, E, float(a), float(b), float(c))
    return out


def rectify(img, rec, border=0):
    """One image through one rectification record (stm_rectify, include/stm_rectify.h; an addition, the reference takes rectified
    pairs): img [H][W][E] sampled bilinearly, in 1/32 pixel, where the record's camera model puts each output pixel; border 0 =
    taps outside the image are 0, 1 = their coordinates are clamped.  rec: 18 floats (stm_amd.rectify.record).  Returns the
    [H][W][E] image (bytes of a pixel past the third are 0); nothing passed in is modified."""
    img, pi = _u8(img)
    H, W, E = img.shape
    rec, pr = _f32(rec)
    assert rec.shape == (18,)
    out = np.zeros((H, W, E), np.uint8)
    lib().stm_rectify(out.ctypes.data_as(u8p), pi, pr, H, W, E, int(border))
    return out


def rectify_coords(rec, num_rows, num_cols):
    """The test tap on the record's coordinate chain (stm_rectify_coords): int32 [H][W][2] of (qu, qv), the source position in 1/32
    pixel, both INT32_MIN where the pixel is not ok."""
    rec, pr = _f32(rec)
    assert rec.shape == (18,)
    quv = np.zeros((int(num_rows), int(num_cols), 2), np.int32)
    lib().stm_rectify_coords(quv.ctypes.data_as(C.POINTER(C.c_int)), pr, int(num_rows), int(num_cols))
    return quv


def align_fit(img_l, img_r, radius=16, rate=1.0, state=None):
    """The measurement of the automatic alignment (stm_align_fit): the vertical offset field a + b u + c v at which the right
    image's content matches the left image's rows, from the SADs of band profiles over +-radius rows, folded into `state` =
    (valid, a, b, c) (None = no history).  Returns (state, valid_blocks): the new state as a float32 array of four and the number
    of the 32 blocks that took part; nothing passed in is modified."""
    img_l, pl = _u8(img_l)
    img_r, pr = _u8(img_r)
    H, W, E = img_l.shape
    assert img_r.shape == (H, W, E)
    st = np.zeros(4, np.float32) if state is None else np.array(state, dtype=np.float32, order="C")
    assert st.shape == (4,)
    n = int(lib().stm_align_fit(pl, pr, H, W, E, int(radius), float(rate), st.ctypes.data_as(f32p)))
    return st, n


def balance_fit(img_l, img_r, max_shift=48, rate=1.0, state=None):
    """The measurement of the colour balance between the eyes (stm_balance_fit; an addition, the reference takes graded pairs): the
    three per-channel tables that bring the right image's histograms onto the left image's, folded into `state` = (valid, 768 levels
    in 1/256) (None = no history).  Returns the new state as an int32 array of 769; nothing passed in is modified."""
    img_l, pl = _u8(img_l)
    img_r, pr = _u8(img_r)
    H, W, E = img_l.shape
    assert img_r.shape == (H, W, E)
    st = np.zeros(769, np.int32) if state is None else np.array(state, dtype=np.int32, order="C")
    assert st.shape == (769,)
    if int(lib().stm_balance_fit(pl, pr, H, W, E, int(max_shift), float(rate), st.ctypes.data_as(C.POINTER(C.c_int)))) != 0:
        raise ValueError("stm_balance_fit refused: %s" % lib().stm_last_error().decode())
    return st


def balance_lut(state):
    """the (3, 256) uint8 tables of a state: clamp((level + 128) >> 8, 0, 255) (stm_balance_apply's step 7)"""
    st = np.asarray(state, np.int32)[1:].astype(np.int64)
    return np.clip((st + 128) >> 8, 0, 255).astype(np.uint8).reshape(3, 256)


def balance_apply(img, lut=None, state=None):
    """The colour balance applied to one image (stm_balance_apply): the first three bytes of every pixel of img [H][W][E] through
    the tables -- lut, uint8 (3, 256) in B, G, R order, or those of state (int32, 769): exactly one of the two.  Returns the
    [H][W][E] image (bytes of a pixel past the third are 0); nothing passed in is modified."""
    img, pi = _u8(img)
    H, W, E = img.shape
    out = np.zeros((H, W, E), np.uint8)
    pl = ps = None
    if lut is not None:
        lut = np.ascontiguousarray(lut, dtype=np.uint8)
        assert lut.size == 768
        pl = lut.ctypes.data_as(u8p)
    if state is not None:
        state = np.ascontiguousarray(state, dtype=np.int32)
        assert state.shape == (769,)
        ps = state.ctypes.data_as(C.POINTER(C.c_int))
    lib().stm_balance_apply(out.ctypes.data_as(u8p), pi, H, W, E, pl, ps)
    return out


def cut_detect(img_l, thresh_permille=370, min_gap=1, state=None):
    """The shot-change detector on one left image (stm_cut_detect; an addition, the reference keeps nothing from frame to frame): the
    image's signature against the one in `state` = (valid, cut, since, score, sig[256]) (None = no history).  Returns (cut, state):
    the flag and the new state as an int32 array of 260; nothing passed in is modified."""
    img_l, pl = _u8(img_l)
    H, W, E = img_l.shape
    st = np.zeros(260, np.int32) if state is None else np.array(state, dtype=np.int32, order="C")
    assert st.shape == (260,)
    cut = int(lib().stm_cut_detect(pl, H, W, E, int(thresh_permille), int(min_gap), st.ctypes.data_as(C.POINTER(C.c_int))))
    if cut < 0:
        raise ValueError("stm_cut_detect refused: %s" % lib().stm_last_error().decode())
    return cut, st


def _rect4(rect):
    return None if rect is None else (C.c_int * 4)(*[int(v) for v in rect])


def active_detect(img_l, thresh_luma=24, lit_permille=10, max_bar_permille=300, hold=12, restart=False, state=None):
    """The active picture area of one left image (stm_active_detect; an addition, the reference measures black bars as picture): the
    rows and columns that hold lit pixels against the bars in `state` = (valid, top, bottom, left, right, changed, H, W, cand[4],
    run[4]) (None = no history).  Returns (changed, state): the flag and the new state as an int32 array of 16, whose words 1 .. 4
    are the rectangle; nothing passed in is modified."""
    img_l, pl = _u8(img_l)
    H, W, E = img_l.shape
    st = np.zeros(16, np.int32) if state is None else np.array(state, dtype=np.int32, order="C")
    assert st.shape == (16,)
    changed = int(lib().stm_active_detect(pl, H, W, E, int(thresh_luma), int(lit_permille), int(max_bar_permille), int(hold), int(bool(restart)),
                                          st.ctypes.data_as(C.POINTER(C.c_int))))
    if changed < 0:
        raise ValueError("stm_active_detect refused: %s" % lib().stm_last_error().decode())
    return changed, st


def active_fill(disp, rect, value):
    """stm_active_fill: the map disp [H][W] with every pixel outside rect = (top, bottom, left, right) set to `value` (None: the map
    as it is).  Returns the new map; nothing passed in is modified."""
    out = np.array(disp, dtype=np.float32, order="C")
    H, W = out.shape
    lib().stm_active_fill(out.ctypes.data_as(f32p), H, W, _rect4(rect), float(value))
    return out


def depth_fit_rect(disp_l, disp_r, disp_lo, disp_hi, max_gain=1.0, clip_permille=20, rate=1.0, state=None, rect=None):
    """depth_fit over the pixels of both maps inside rect = (top, bottom, left, right) only (stm_depth_fit_rect; None = depth_fit)."""
    disp_l, pl = _f32(disp_l)
    disp_r, pr = _f32(disp_r)
    H, W = disp_l.shape
    assert disp_r.shape == (H, W)
    st = np.zeros(4, np.float32) if state is None else np.array(state, dtype=np.float32, order="C")
    assert st.shape == (4,)
    lib().stm_depth_fit_rect(pl, pr, H, W, float(disp_lo), float(disp_hi), float(max_gain), int(clip_permille), float(rate),
                             st.ctypes.data_as(f32p), _rect4(rect))
    return st


def overlay_fit_rect(disp_l, disp_r, overlay, x0, y0, view_rows, view_cols, limit_lo, limit_hi, gain=1.0, conv=0.0, near_permille=20,
                     margin=1.0, pad=8, rate_near=1.0, rate_far=0.1, restart=False, state=None, rect=None):
    """overlay_fit with the footprint's map rectangle moved into rect = (top, bottom, left, right) (stm_overlay_fit_rect; None =
    overlay_fit)."""
    disp_l, pl = _f32(disp_l)
    disp_r, pr = _f32(disp_r)
    overlay, po = _u8(overlay)
    H, W = disp_l.shape
    assert disp_r.shape == (H, W) and overlay.ndim == 3 and overlay.shape[2] == 4
    st = np.zeros(4, np.float32) if state is None else np.array(state, dtype=np.float32, order="C")
    assert st.shape == (4,)
    lib().stm_overlay_fit_rect(pl, pr, H, W, po, overlay.shape[0], overlay.shape[1], int(x0), int(y0), int(view_rows), int(view_cols),
                               float(gain), float(conv), int(near_permille), float(margin), int(pad), float(limit_lo), float(limit_hi),
                               float(rate_near), float(rate_far), int(bool(restart)), st.ctypes.data_as(f32p), _rect4(rect))
    return st


def tx_scale(img, out_rows, out_cols):
    """d_tx_scale.h:17-18 (bilinear resize)."""
    img, pi = _u8(img)
    H, W, E = img.shape
    out = np.zeros((out_rows, out_cols, E), np.uint8)
    lib().stm_d_tx_scale(pi, out.ctypes.data_as(u8p), H, W, out_rows, out_cols, E)
    return out


def bmp_read(path):
    """stm_bmp_read: the C++ twin of bmp_io.read_bmp (replaces cv::imread, image_io.cpp:95-96)."""
    h, w = C.c_int(0), C.c_int(0)
    p = lib().stm_bmp_read(path.encode(), C.byref(h), C.byref(w))
    if not p:
        raise IOError("stm_bmp_read failed for %s" % path)
    try:
        arr = np.ctypeslib.as_array(C.cast(p, u8p), shape=(h.value, w.value, 3)).copy()
    finally:
        lib().stm_bmp_free(p)
    return arr


def bmp_write(path, img):
    img, pi = _u8(img)
    if lib().stm_bmp_write(path.encode(), pi, img.shape[0], img.shape[1]) != 0:
        raise IOError("stm_bmp_write failed for %s" % path)


def demux_nv12(y, uv, num_cols, elem_sz=3, matrix=0, num_cols_sbs=None):
    """stm_demux_nv12: the two views (each uint8 [H][num_cols][elem_sz], BGR in the first three bytes, 0 past them) of a
    side-by-side NV12 frame.  y uint8 [H][>= Wsbs] and uv uint8 [H / 2][>= Wsbs] are 2-D arrays whose row stride is the plane's
    pitch (a view into a larger buffer is fine); matrix: 0 / 1 = BT.601 / BT.709 limited range, 2 / 3 = BT.601 / BT.709 full."""
    for a in (y, uv):
        assert a.dtype == np.uint8 and a.ndim == 2 and (a.shape[1] == 1 or a.strides[1] == 1)
    H = y.shape[0]
    Wsbs = y.shape[1] if num_cols_sbs is None else num_cols_sbs
    assert uv.shape[0] * 2 == H and y.shape[1] >= Wsbs and uv.shape[1] >= 2 * ((Wsbs + 1) // 2)
    img_l = np.zeros((H, num_cols, elem_sz), np.uint8)
    img_r = np.zeros_like(img_l)
    lib().stm_demux_nv12(img_l.ctypes.data_as(u8p), img_r.ctypes.data_as(u8p), y.ctypes.data_as(u8p), y.strides[0],
                         uv.ctypes.data_as(u8p), uv.strides[0], H, Wsbs, num_cols, elem_sz, int(matrix))
    return img_l, img_r


def mux_nv12(img, matrix=0, pitch_y=None, pitch_uv=None):
    """stm_mux_nv12: the NV12 picture (y uint8 [H][pitch_y], uv uint8 [H / 2][pitch_uv]; the samples in the first W bytes of a row, 0
    past them) of the BGR image img uint8 [H][W][E], H and W even: 16.16 integer luma, chroma the mean of each 2 x 2 block.  matrix:
    0 / 1 = BT.601 / BT.709 limited range, 2 / 3 = BT.601 / BT.709 full range; the pitches default to W."""
    img, pi = _u8(img)
    H, W, E = img.shape
    pitch_y, pitch_uv = pitch_y or W, pitch_uv or W
    y = np.zeros((H, max(pitch_y, 1)), np.uint8)
    uv = np.zeros((max(H // 2, 1), max(pitch_uv, 1)), np.uint8)
    lib().stm_mux_nv12(y.ctypes.data_as(u8p), pitch_y, uv.ctypes.data_as(u8p), pitch_uv, pi, H, W, E, int(matrix))
    return y, uv


def demux_packed(img, num_rows, num_cols, packing, elem_sz=None):
    """stm_demux_packed: the two unpacked eyes (each uint8 [num_rows][num_cols][E], BGR in the first three bytes, 0 past them) of a
    packed BGR frame img uint8 [rows_f][Wsbs][E] (contiguous); packing = (packing, swap, filter, gap), stm_set_packing's settings."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.ndim == 3
    E = img.shape[2] if elem_sz is None else elem_sz
    img_l = np.zeros((num_rows, num_cols, E), np.uint8)
    img_r = np.zeros_like(img_l)
    pk, sw, fl, gap = (int(v) for v in packing)
    lib().stm_demux_packed(img_l.ctypes.data_as(u8p), img_r.ctypes.data_as(u8p), img.ctypes.data_as(u8p), num_rows, img.shape[1], num_cols,
                           E, pk, sw, fl, gap)
    return img_l, img_r


def demux_nv12_packed(y, uv, num_rows, num_cols, packing, elem_sz=3, matrix=0, num_cols_sbs=None):
    """stm_demux_nv12_packed: demux_packed on a packed NV12 frame: y uint8 [rows_f][>= Wsbs], uv uint8 [rows_f / 2][>= Wsbs], planes
    as for demux_nv12 (the row stride is the pitch)."""
    for a in (y, uv):
        assert a.dtype == np.uint8 and a.ndim == 2 and (a.shape[1] == 1 or a.strides[1] == 1)
    Wsbs = y.shape[1] if num_cols_sbs is None else num_cols_sbs
    assert uv.shape[0] * 2 == y.shape[0] and y.shape[1] >= Wsbs and uv.shape[1] >= 2 * ((Wsbs + 1) // 2)
    img_l = np.zeros((num_rows, num_cols, elem_sz), np.uint8)
    img_r = np.zeros_like(img_l)
    pk, sw, fl, gap = (int(v) for v in packing)
    lib().stm_demux_nv12_packed(img_l.ctypes.data_as(u8p), img_r.ctypes.data_as(u8p), y.ctypes.data_as(u8p), y.strides[0],
                                uv.ctypes.data_as(u8p), uv.strides[0], num_rows, Wsbs, num_cols, elem_sz, int(matrix), pk, sw, fl, gap)
    return img_l, img_r


def demux_sbs_low(img_sbs, num_cols, disp_rows, disp_cols, census=True):
    """stm_demux_sbs_low: the reduced-resolution frame's front on host arrays.  img_sbs uint8 [H][Wsbs][E] (contiguous).  Returns
    (img_l, img_r, low_l, low_r, census_l, census_r): the split images [H][num_cols][E], the bilinearly reduced images
    [disp_rows][disp_cols][E] (BGR in the first three bytes, 0 past them) and the reduced images' 32-bit census words (uint32
    [disp_rows][disp_cols]; None, None with census=False)."""
    img_sbs = np.ascontiguousarray(img_sbs, dtype=np.uint8)
    H, Wsbs, E = img_sbs.shape
    img_l = np.zeros((H, num_cols, E), np.uint8)
    img_r = np.zeros_like(img_l)
    low_l = np.zeros((disp_rows, disp_cols, E), np.uint8)
    low_r = np.zeros_like(low_l)
    cen_l = np.zeros((disp_rows, disp_cols), np.uint32) if census else None
    cen_r = np.zeros((disp_rows, disp_cols), np.uint32) if census else None
    lib().stm_demux_sbs_low(img_l.ctypes.data_as(u8p), img_r.ctypes.data_as(u8p), low_l.ctypes.data_as(u8p), low_r.ctypes.data_as(u8p),
                            cen_l.ctypes.data_as(u32p) if census else None, cen_r.ctypes.data_as(u32p) if census else None,
                            img_sbs.ctypes.data_as(u8p), H, Wsbs, num_cols, disp_rows, disp_cols, E)
    return img_l, img_r, low_l, low_r, cen_l, cen_r
