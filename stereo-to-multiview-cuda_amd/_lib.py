"""Loader + ctypes prototypes for libstm_hip.so (include/stm_hip.h).

There is deliberately no CPU fallback: if the HIP library is missing, importing a stage raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libstm_hip.so")
# STM_LIB=timing: the tools/*_time.py experiments load the -DSTM_TIMING build of the same sources (kernels with parts
# switched off; results NOT valid).  Nothing else ever loads it.
if os.environ.get("STM_LIB") == "timing":
    LIB_PATH = os.path.join(HERE, "libstm_hip_timing.so")

u8p = C.POINTER(C.c_uint8)
f32p = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)
u8pp = C.POINTER(u8p)
f32pp = C.POINTER(f32p)
vp = C.c_void_p
i, f, d = C.c_int, C.c_float, C.c_double

# name -> argtypes, in the order of include/stm_hip.h.  Device-flavour entries take raw addresses (c_void_p).
PROTOS = {
    "stm_version": ([], i),
    "stm_set_stream": ([vp], None),
    "stm_get_stream": ([], vp),
    "stm_set_error_mode": ([i], None),
    "stm_last_error": ([], C.c_char_p),
    "stm_release_workspace": ([], None),
    "stm_prof_enable": ([i], None),
    "stm_prof_reset": ([], None),
    "stm_prof_read": ([C.c_char_p, f32p], i),
    "stm_set_agg_variant": ([i], None),
    "stm_agg_path": ([i, i, i, i, i, i], i),
    "stm_first_pass_path": ([i, i, i, i, i, i], i),
    "stm_px_order": ([i, i, i, i, i, i], i),
    "stm_set_agg_tap": ([vp, vp, vp, vp], i),
    "stm_set_irv_paper_ratio": ([i], None),
    "stm_set_irv_chunk": ([i], i),
    "stm_irv_path": ([i, i, i, i, i, i], i),
    "stm_set_ref_quirks": ([i], None),
    "stm_set_lens": ([i, d, d, d], i),
    "stm_set_layout": ([i, i, i, i, i], i),
    "stm_get_layout": ([C.POINTER(C.c_int)], None),
    "stm_set_output": ([i, i, i, i], i),
    "stm_get_output": ([C.POINTER(C.c_int)], None),
    "stm_set_overlay": ([i, vp, i, i, i, i, f], i),
    "stm_get_overlay": ([C.POINTER(C.c_int), f32p], None),
    "stm_set_overlay_auto": ([i, i, f, i, f, f, f, f, vp], i),
    "stm_get_overlay_auto": ([C.POINTER(C.c_int), f32p], None),
    "stm_set_quilt_lds_limit": ([i], None),
    "stm_set_packing": ([i, i, i, i], i),
    "stm_get_packing": ([C.POINTER(C.c_int)], None),
    "stm_set_depth": ([i, f, f], i),
    "stm_set_depth_auto": ([f, f, f, i, f, vp], i),
    "stm_set_antialias": ([i, f, i, f], i),
    "stm_get_antialias": ([C.POINTER(C.c_int), f32p], None),
    "stm_set_align": ([i, f, f, f], i),
    "stm_set_align_auto": ([i, f, vp], i),
    "stm_get_align": ([C.POINTER(C.c_int), f32p], None),
    "stm_set_balance": ([i, u8p], i),
    "stm_set_balance_auto": ([i, f, vp], i),
    "stm_get_balance": ([C.POINTER(C.c_int), f32p, u8p], None),
    "stm_set_cut": ([i, i, i, vp], i),
    "stm_get_cut": ([C.POINTER(C.c_int)], None),
    "stm_set_active": ([i, C.POINTER(C.c_int), i, f], i),
    "stm_set_active_auto": ([i, i, i, i, vp], i),
    "stm_get_active": ([C.POINTER(C.c_int), f32p], None),
    "stm_ci_adcensus": ([u8p, u8p, f32pp, f32pp, f, f, i, i, i, i, i], None),
    "stm_d_ci_adcensus": ([vp, vp, vp, vp, f32pp, f32pp, vp, f, f, i, i, i, i, i], None),
    "stm_ca_cross": ([u8p, u8pp, f32pp, f32pp, f, f, i, i, i, i, i, i], None),
    "stm_d_ca_cross": ([vp, vp, vp, f32pp, vp, vp, f, f, i, i, i, i, i, i], None),
    "stm_dc_wta": ([f32pp, f32p, i, i, i, i], None),
    "stm_d_dc_wta": ([vp, vp, i, i, i, i], None),
    "stm_dc_subpixel": ([f32pp, f32p, i, i, i, i], None),
    "stm_d_dc_subpixel": ([vp, vp, i, i, i, i], None),
    "stm_dc_hslo": ([f32pp, f32p, u8p, u8p, f, f, f, i, i, i, i, i], None),
    "stm_d_dc_hslo": ([vp, vp, vp, vp, f, f, f, i, i, i, i, i], None),
    "stm_dr_dcc": ([u8p, u8p, f32p, f32p, i, i], None),
    "stm_d_dr_dcc": ([vp, vp, vp, vp, i, i], None),
    "stm_dr_irv": ([f32p, u8p, u8pp, i, f, i, i, i, i, i, i], None),
    "stm_d_dr_irv": ([vp, vp, vp, i, f, i, i, i, i, i, i], None),
    "stm_dr_interp": ([f32p, u8p, u8p, i, i, i], None),
    "stm_d_dr_interp": ([vp, vp, vp, i, i, i], None),
    "stm_filter_bilateral_1": ([f32p, i, f, f, i, i, i], None),
    "stm_d_filter_bilateral_1": ([vp, i, f, f, i, i, i], None),
    "stm_filter_gaussian_1": ([f32p, i, f, i, i], None),
    "stm_d_filter_gaussian_1": ([vp, i, f, i, i], None),
    "stm_filter_bleed_1": ([u8p, i, i, i], None),
    "stm_d_filter_bleed_1": ([vp, i, i, i], None),
    "stm_filter_median": ([f32p, i, i], None),
    "stm_generate_gaussian_kernel": ([f32p, i, f], None),
    "stm_d_filter_median": ([vp, i, i], None),
    "stm_dibr_occl": ([u8p, u8p, f32p, f32p, i, i], None),
    "stm_d_dibr_occl": ([vp, vp, vp, vp, i, i], None),
    "stm_dibr_occl_to_mask": ([f32p, f32p, u8p, u8p, i, i], None),
    "stm_d_dibr_occl_to_mask": ([vp, vp, vp, vp, i, i], None),
    "stm_dibr_dbm": ([u8p, u8p, u8p, f32p, f32p, u8p, u8p, f32p, f32p, f, i, i, i], None),
    "stm_d_dibr_dbm": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, f, i, i, i], None),
    "stm_dibr_dbm_lin": ([u8p, u8p, u8p, f32p, f32p, u8p, u8p, f32p, f32p, f, i, i, i], None),
    "stm_d_dibr_dbm_lin": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, f, i, i, i], None),
    "stm_dibr_dfm": ([u8p, u8p, u8p, f32p, f32p, f, i, i, i], None),
    "stm_d_dibr_dfm": ([vp, vp, vp, vp, vp, f, i, i, i], None),
    "stm_mux_multiview": ([u8pp, u8p, i, f, i, i, i, i, i], None),
    "stm_d_mux_multiview": ([vp, vp, i, f, i, i, i, i, i], None),
    "stm_mux_multiview_lens": ([u8pp, u8p, i, i, d, d, d, i, i, i, i, i], None),
    "stm_d_mux_multiview_lens": ([vp, vp, i, i, d, d, d, i, i, i, i, i], None),
    "stm_quilt_multiview": ([u8pp, u8p, i, i, i, i, i, i, i, i, i, i], None),
    "stm_d_quilt_multiview": ([vp, vp, i, i, i, i, i, i, i, i, i, i], None),
    "stm_mux_overlay": ([u8p, u8p, i, i, i, i, f, i, f, i, d, d, d, i, i, i, i, i, i, i], None),
    "stm_d_mux_overlay": ([vp, vp, i, i, i, i, f, i, f, i, d, d, d, i, i, i, i, i, i, i], None),
    "stm_d_demux_sbs": ([vp, vp, vp, i, i, i, i], None),
    "stm_demux_nv12": ([u8p, u8p, u8p, i, u8p, i, i, i, i, i, i], None),
    "stm_d_demux_nv12": ([vp, vp, vp, i, vp, i, i, i, i, i, i], None),
    "stm_mux_nv12": ([u8p, i, u8p, i, u8p, i, i, i, i], None),
    "stm_d_mux_nv12": ([vp, i, vp, i, vp, i, i, i, i], None),
    "stm_demux_packed": ([u8p, u8p, u8p, i, i, i, i, i, i, i, i], None),
    "stm_d_demux_packed": ([vp, vp, vp, i, i, i, i, i, i, i, i], None),
    "stm_demux_nv12_packed": ([u8p, u8p, u8p, i, u8p, i, i, i, i, i, i, i, i, i, i], None),
    "stm_d_demux_nv12_packed": ([vp, vp, vp, i, vp, i, i, i, i, i, i, i, i, i, i], None),
    "stm_adcensus_stm": ([u8p, f32p, f32p, u8p, i, i, i, i, i, i, i, f, i, i, f, f, f, f, i, i, i, f], None),
    "stm_d_adcensus_stm": ([vp, vp, vp, vp, i, i, i, i, i, i, i, f, i, i, f, f, f, f, i, i, i, f, i], None),
    "stm_d_adcensus_stm_t": ([vp, vp, vp, vp, i, i, i, i, i, i, i, f, i, i, f, f, f, f, i, i, i, f, i, vp, vp, vp, f, i, f], None),
    "stm_d_adcensus_stm_nv12": ([vp, i, vp, i, i, vp, vp, vp, i, i, i, i, i, i, i, f, i, i, f, f, f, f, i, i, i, f, i, vp, vp, vp, vp, f, i, f,
                                 vp, vp], None),
    "stm_adcensus_stm_2": ([u8p, f32p, f32p, u8p, i, i, i, i, i, i, i, i, f, i, f, i, i, f, f, f, f, i, i, i, f], None),
    "stm_d_adcensus_stm_2": ([vp, vp, vp, vp, i, i, i, i, i, i, i, i, f, i, f, i, i, f, f, f, f, i, i, i, f], None),
    "stm_adcensus_stm_2s": ([u8p, f32p, f32p, u8p, i, i, i, i, i, i, i, i, f, i, f, i, i, f, f, f, f, i, i, i, f, i], None),
    "stm_d_adcensus_stm_2s": ([vp, vp, vp, vp, i, i, i, i, i, i, i, i, f, i, f, i, i, f, f, f, f, i, i, i, f, i], None),
    "stm_d_adcensus_stm_2t": ([vp, vp, vp, vp, i, i, i, i, i, i, i, i, f, i, f, i, i, f, f, f, f, i, i, i, f, i, vp, vp, vp, f, i, f], None),
    "stm_d_adcensus_stm_2nv12": ([vp, i, vp, i, i, vp, vp, vp, i, i, i, i, i, i, i, i, f, i, f, i, i, f, f, f, f, i, i, i, f, i, vp, vp, vp, vp,
                                  f, i, f, vp, vp], None),
    "stm_demux_sbs_low": ([u8p, u8p, u8p, u8p, u32p, u32p, u8p, i, i, i, i, i, i], None),
    "stm_d_demux_sbs_low": ([vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i], None),
    "stm_demux_nv12_low": ([u8p, u8p, u8p, u8p, u32p, u32p, u8p, i, u8p, i, i, i, i, i, i, i, i], None),
    "stm_d_demux_nv12_low": ([vp, vp, vp, vp, vp, vp, vp, i, vp, i, i, i, i, i, i, i, i], None),
    "stm_disp_upsample": ([f32p, f32p, u8p, u8p, i, i, i, i, i, f, f], None),
    "stm_d_disp_upsample": ([vp, vp, vp, vp, i, i, i, i, i, f, f], None),
    "stm_disp_temporal": ([f32p, f32p, u8p, u8p, i, i, i, f, i, f], None),
    "stm_d_disp_temporal": ([vp, vp, vp, vp, i, i, i, f, i, f], None),
    "stm_depth_fit": ([f32p, f32p, i, i, f, f, f, i, f, f32p], None),
    "stm_d_depth_fit": ([vp, vp, i, i, f, f, f, i, f, vp], None),
    "stm_overlay_fit": ([f32p, f32p, i, i, u8p, i, i, i, i, i, i, f, f, i, f, i, f, f, f, f, i, f32p], None),
    "stm_d_overlay_fit": ([vp, vp, i, i, vp, i, i, i, i, i, i, f, f, i, f, i, f, f, f, f, i, vp, vp], None),
    "stm_align_rows": ([u8p, u8p, i, i, i, f, f, f], None),
    "stm_d_align_rows": ([vp, vp, i, i, i, f, f, f], None),
    "stm_align_fit": ([u8p, u8p, i, i, i, i, f, f32p], i),
    "stm_d_align_fit": ([vp, vp, i, i, i, i, f, vp, vp, vp, vp], None),
    "stm_balance_fit": ([u8p, u8p, i, i, i, i, f, C.POINTER(C.c_int)], i),
    "stm_d_balance_fit": ([vp, vp, i, i, i, i, f, vp, vp], None),
    "stm_balance_apply": ([u8p, u8p, i, i, i, u8p, C.POINTER(C.c_int)], None),
    "stm_d_balance_apply": ([vp, vp, i, i, i, u8p, vp], None),
    "stm_cut_detect": ([u8p, i, i, i, i, i, C.POINTER(C.c_int)], i),
    "stm_d_cut_detect": ([vp, i, i, i, i, i, vp, vp, vp, vp, vp], None),
    "stm_active_detect": ([u8p, i, i, i, i, i, i, i, i, C.POINTER(C.c_int)], i),
    "stm_d_active_detect": ([vp, i, i, i, i, i, i, i, i, vp, vp, vp], None),
    "stm_active_fill": ([f32p, i, i, C.POINTER(C.c_int), f], None),
    "stm_d_active_fill": ([vp, i, i, vp, f], None),
    "stm_depth_fit_rect": ([f32p, f32p, i, i, f, f, f, i, f, f32p, C.POINTER(C.c_int)], None),
    "stm_d_depth_fit_rect": ([vp, vp, i, i, f, f, f, i, f, vp, vp], None),
    "stm_overlay_fit_rect": ([f32p, f32p, i, i, u8p, i, i, i, i, i, i, f, f, i, f, i, f, f, f, f, i, f32p, C.POINTER(C.c_int)], None),
    "stm_d_overlay_fit_rect": ([vp, vp, i, i, vp, i, i, i, i, i, i, f, f, i, f, i, f, f, f, f, i, vp, vp, vp], None),
    "stm_view_prefilter": ([u8p, u8p, f32p, i, i, i, i, f, i, f, f, f], None),
    "stm_d_view_prefilter": ([vp, vp, vp, i, i, i, i, f, i, f, f, f], None),
    "stm_d_tx_scale": ([u8p, u8p, i, i, i, i, i], None),
    "stm_stream_create": ([i, i, i, i, i, i, i, f, i, i, f, f, f, f, i, i, i, f], C.c_void_p),
    "stm_stream_submit": ([C.c_void_p, u8p], C.c_long),
    "stm_stream_set_stages": ([C.c_void_p, i], i),
    "stm_stream_set_match_size": ([C.c_void_p, i, i, f], i),
    "stm_stream_set_temporal": ([C.c_void_p, f, i, f], i),
    "stm_stream_set_input": ([C.c_void_p, i, i], i),
    "stm_stream_set_packing": ([C.c_void_p, i, i, i, i], i),
    "stm_stream_set_lens": ([C.c_void_p, i, d, d, d], i),
    "stm_stream_set_layout": ([C.c_void_p, i, i, i, i, i], i),
    "stm_stream_set_output": ([C.c_void_p, i, i], i),
    "stm_stream_set_overlay": ([C.c_void_p, i, i], i),
    "stm_stream_overlay": ([C.c_void_p, u8p, i, i, i, i, f], i),
    "stm_stream_set_overlay_auto": ([C.c_void_p, i, i, f, i, f, f, f, f], i),
    "stm_stream_overlay_depth": ([C.c_void_p, f32p], i),
    "stm_stream_set_depth": ([C.c_void_p, i, f, f], i),
    "stm_stream_set_depth_auto": ([C.c_void_p, f, f, f, i, f], i),
    "stm_stream_set_antialias": ([C.c_void_p, i, f, i, f], i),
    "stm_stream_depth": ([C.c_void_p, f32p], i),
    "stm_stream_set_align": ([C.c_void_p, i, f, f, f], i),
    "stm_stream_set_align_auto": ([C.c_void_p, i, f], i),
    "stm_stream_align": ([C.c_void_p, f32p], i),
    "stm_stream_set_balance": ([C.c_void_p, i, u8p], i),
    "stm_stream_set_balance_auto": ([C.c_void_p, i, f], i),
    "stm_stream_balance": ([C.c_void_p, u8p], i),
    "stm_stream_set_cut": ([C.c_void_p, i, i, i], i),
    "stm_stream_cut": ([C.c_void_p, C.POINTER(C.c_int)], i),
    "stm_stream_set_active": ([C.c_void_p, i, C.POINTER(C.c_int), i, f, i, i, i, i], i),
    "stm_stream_active": ([C.c_void_p, C.POINTER(C.c_int)], i),
    "stm_stream_collect": ([C.c_void_p, f32p, f32p, u8p], C.c_long),
    "stm_stream_input_buffer": ([C.c_void_p], C.c_void_p),
    "stm_stream_collect_view": ([C.c_void_p, C.POINTER(f32p), C.POINTER(f32p), C.POINTER(u8p)], C.c_long),
    "stm_stream_maps": ([C.c_void_p, i, i, f, f], i),
    "stm_stream_collect_maps": ([C.c_void_p, C.c_void_p, C.c_void_p, u8p], C.c_long),
    "stm_stream_collect_maps_view": ([C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(u8p)], C.c_long),
    "stm_stream_destroy": ([C.c_void_p], None),
    "stm_bmp_read": ([C.c_char_p, C.POINTER(i), C.POINTER(i)], C.c_void_p),
    "stm_bmp_write": ([C.c_char_p, u8p, i, i], i),
    "stm_bmp_free": ([C.c_void_p], None),
}
# include/stm_depth_input.h: the entry of a frame stream's image-plus-depth input.  PROTOS is include/stm_hip.h, name for name, and that
# header's names are recorded in the test suite's screening tables, so a later stream entry has its own header and its own table
PROTOS_DEPTH = {
    "stm_stream_input_depth": ([C.c_void_p, i, f, f, i, f], i),
}
# include/stm_rectify.h: rectification from camera calibration, likewise in a header and a table of its own
PROTOS_RECTIFY = {
    "stm_rectify": ([u8p, u8p, f32p, i, i, i, i], None),
    "stm_d_rectify": ([vp, vp, f32p, i, i, i, i], None),
    "stm_rectify_coords": ([C.POINTER(C.c_int), f32p, i, i], None),
    "stm_stream_rectify": ([C.c_void_p, i, f32p, i], i),
    "stm_stream_get_rectify": ([C.c_void_p, C.POINTER(C.c_int), f32p, C.POINTER(C.c_int)], i),
}
# include/stm_hslo_tap.h: the test tap on the scanline passes' sums and the right view as a stage, likewise
PROTOS_HSLO = {
    "stm_set_hslo_tap": ([vp, vp, vp], i),
    "stm_d_dc_hslo_view": ([vp, vp, vp, vp, f, f, f, i, i, i, i, i, i], None),
}
# include/stm_depth_video.h: packed 2D-plus-depth video frames as a frame stream's input, likewise
PROTOS_DEPTH_VIDEO = {
    "stm_stream_input_packed_depth": ([C.c_void_p, i, i, i, i, i, i, i, i, i, f, f, i, f], i),
}

_lib = None


def lib():
    """The loaded C-ABI library.  Raises (no fallback) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libstm_hip.so is missing (%s): build it with __graft_entry__.build() / make -C csrc; "
                "there is no CPU fallback for the product path" % LIB_PATH)
        # torch bundles its own libamdhip64.so.7; it must be in the process BEFORE this library is loaded so that
        # both share ONE HIP runtime (same device context, torch streams valid for stm_set_stream).  Loading in the
        # other order starts two runtimes and the second one finds "no ROCm-capable device".
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (args, res) in list(PROTOS.items()) + list(PROTOS_DEPTH.items()) + list(PROTOS_RECTIFY.items()) + list(PROTOS_HSLO.items()) + list(PROTOS_DEPTH_VIDEO.items()):
            fn = getattr(l, name)
            fn.argtypes = args
            fn.restype = res
        _lib = l
    return _lib
