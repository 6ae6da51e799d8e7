/*
 * stm_hip.h -- C ABI of the MI355X-native stereo->multiview hot path (libstm_hip.so).
 *
 * Every entry point below replaces one function of the reference's per-stage host
 * API.  The reference relies on C++ name mangling and has no
 * C ABI, so each function is exported here as  stm_<reference name>  with the
 * reference's argument list unchanged (same order, same meaning, same ownership):
 *   - "host flavour"   stm_xxx   : every pointer is a HOST pointer; the call uploads,
 *                                   runs the HIP kernels, downloads and returns only
 *                                   when the outputs are visible to the host.
 *   - "device flavour" stm_d_xxx : every pointer is a DEVICE pointer (plus the host
 *                                   mirror tables the reference also passes); kernels
 *                                   are enqueued on the current stream (stm_set_stream),
 *                                   nothing is synchronised.
 * C++ callers that want the reference's exact (mangled) names -- image_io.cpp /
 * d_io.cu style call sites -- include stm_dropin.hpp instead.
 *
 * Layouts (reference: image_io.cpp:155-189, d_io.cu:71-101):
 *   images      interleaved BGR u8, row-major, no row padding, elem_sz == 3 in the reference's drivers; any elem_sz >= 3 is
 *               accepted: bytes 0..2 of a pixel are read and written, and the padding bytes (3 .. elem_sz-1) of an output
 *               image are 0 after a host-flavour call, untouched by a device-flavour call -- except stm_d_dibr_dbm and
 *               stm_d_dibr_dfm, which clear their whole output image like the reference (d_dibr_bwarp.cu:53, d_dibr_fwarp.cu:51,84)
 *   cost volume table of num_disp pointers, each a dense num_rows*num_cols float plane
 *   cross arms  table of 4 pointers to u8 planes, order UP, DOWN, LEFT, RIGHT
 *   disparity   float [H][W], signed offset (d - zero_disp)
 *
 * Threading: the reference is single-threaded on the default stream.  Here every host thread has
 * its own current stream (stm_set_stream) and its own cached workspace per device, so threads may call into the
 * library concurrently; device-flavour calls of two threads that touch the same buffers need streams ordered by
 * the caller.  A thread that ends should call stm_release_workspace() first (its slab is not freed for it).
 *
 * Errors: like the reference (cuda_utils.h:12-21) a HIP failure prints a message and
 * calls exit(1); unlike it, kernel launches are checked too.  stm_set_error_mode(1)
 * turns that into "record and return" for embedding hosts (query stm_last_error()).
 * Arguments the reference would turn into undefined behaviour are errors of the same kind:
 * a dimension < 1, elem_sz < 3 (three channels of every element are read), num_views < 2
 * for the interlacer (d_mux_multiview.cu:62-66 reads views[1]), an angle whose row period
 * round(num_views / tan(angle) / elem_sz) is 0 (ty % 0, :55) or not finite (tan(angle) == 0, :146),
 * num_cols > 8192 in ca_cross.
 *
 * All file:line citations are relative to the reference repository root.
 */
#ifndef STM_HIP_H
#define STM_HIP_H

#ifdef __cplusplus
extern "C" {
#endif
#if defined(STM_BUILD) && defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---------------------------------------------------------------- runtime */
int         stm_version(void);
/* current HIP stream (a hipStream_t) used by every device-flavour call of this thread */
void        stm_set_stream(void *hip_stream);
void       *stm_get_stream(void);
/* 0 = print + exit(1) like cuda_utils.h:12-21 (default); 1 = record, return, keep going */
void        stm_set_error_mode(int mode);
/* the calling thread's last error text.  It also waits for the thread's stream and reads (and clears) a device-side word that
 * the region-voting kernels set if they had to clamp their outlier list -- a condition that cannot arise while the library
 * clears its counters per call, reported instead of swallowed if it ever does. */
const char *stm_last_error(void);
/* frees the cached device workspace (the reference cudaMalloc/cudaFree's per call) */
void        stm_release_workspace(void);
/* per-kernel HIP-event profiling of the named kernels inside the frame pipeline: 0 off, 1 every named kernel,
 * 2 the aggregation kernels only (three event pairs per frame: what bench.py keeps on inside its timed region) */
void        stm_prof_enable(int on);
void        stm_prof_reset(void);
/* returns number of timed launches of `kernel` ("pq_h","pq_v12","pq_hw","cross_arms","irv","hslo_lr","hslo_rl","hslo_tb",
 * "hslo_bt", "subpixel", "interp", "upsample", "temporal", ...) and their
 * summed duration in ms; synchronises the recorded events. */
int         stm_prof_read(const char *kernel, float *total_ms);
/* aggregation variant of the frame pipeline (0 = default: matrix-pipe kernels, stm_kernels_aggm.hip); decimal digits, used by
 * the benchmark and the tools to A/B result-preserving variants in one process: 10000 = vector-ALU aggregation kernels
 * (stm_kernels_agg.hip; the low digits then select their tunables), 1000000 = separate initial-cost kernel instead of
 * computing the costs inside the first pass, 2000000 = the cost-computing first pass with one view per block (stm_k_pq_hc) where
 * the default sweeps both views of a row part from one ring of costs (stm_k_pq_hc2; stm_first_pass_path), 1000 / 2000 = the cost-computing pass as one block per segment (128- / 192-pixel
 * segments) instead of the row walk, 10 = the volume-reading horizontal passes as one block per segment instead of the row walk
 * (20: only for num_disp > 64), 200 = view synthesis and interlacing as two kernels, 300 = region voting over the raster-ordered outlier list of round 3
 * instead of over column runs, 400 = the two horizontal scanline-optimisation passes as two launches instead of one walk from both
 * ends of a row, 500 (tests) = the per-stage filter_bilateral_1 through the frame pipeline's integer-map kernel (which checks each tile
 * of its input and takes the general form where the map is not integer-valued inside the colour table), 600 = the image-sized
 * chain of the frame as separate kernels (split + pixel formats, then census; L/R check, then row counts, then the full-height
 * column prefix, with the vote codes packed by the compaction kernel) instead of the fused front kernel, the fused row kernel and
 * the column sums inside the compaction kernel, 700 = the cross-arm walk with its bookkeeping in vector registers (round 3) instead
 * of in lane masks and scalar row offsets, 800 = the vertical passes of the pixel-major fast path as masked MFMA sweeps with the
 * windows as mask records (stm_k_pq_v12m) instead of as exact runs of vector adds with the arms as a table of jump offsets
 * (stm_k_pq_v12r; the frame stays on the pixel-major volumes and every query below answers as under 0;
 * tests/test_gpu_vertical_vadd.py), 10000000 = the vertical passes on the LDS-ring
 * kernel of round 3 instead of the register-ring kernel (stm_kernels_aggv.hip), 20000000 = the register-ring kernel with a strip of
 * four columns per wave and the PQ volume layout end to end instead of one column per wave on pixel-major volumes (48 < num_disp <= 64
 * only; elsewhere the default already is the former), 100000000 = the last horizontal pass + WTA on the
 * LDS row walk instead of the register-ring kernel (stm_kernels_aggh.hip), 1000000000 = the window tables of the two register-ring
 * kernels from their own launches instead of from the cross-arm kernel, 2000000000 = the pixel-major volumes with a pixel's
 * hypotheses in ascending order and sixteen 4-byte stores per tile in the first pass and in the vertical kernel instead of the orders
 * that let both store 16 bytes at a time (stm_px_order; tests/test_gpu_px_store_order.py).  Every accepted variant produces identical
 * results (tests/test_gpu_parity.py::test_device_frame_agg_variants, tests/test_gpu_image_chain.py,
 * tests/test_gpu_cross_arms.py, tests/test_gpu_px_layout.py).  The
 * digit N00000 (timing experiments that skip parts of kernels) is ignored here: it exists only in libstm_hip_timing.so,
 * a separate build of the same sources with -DSTM_TIMING (csrc/Makefile, `make timing`). */
void        stm_set_agg_variant(int v);
/* Which aggregation kernels a frame call (stm_adcensus_stm, stm_d_adcensus_stm, _t, _nv12; _2 / _2s with the size the match runs
 * at) takes for these arguments under the current stm_set_agg_variant.  Host arithmetic only: nothing is launched, no device is
 * touched, no argument is screened, and the answer comes from the very functions the frame call dispatches through.  num_rows,
 * num_cols: one eye's size; stages: as the frame call takes it.  A bit field:
 *   bit 0        the chain on the matrix pipe (stm_kernels_aggm.hip); 0: the vector-ALU kernels, and every other bit is 0
 *   bit 1        the two intermediate volumes pixel-major (PX): stm_k_pq_hc's PX stores, stm_k_pq_v12r, stm_k_pq_hsr's PX loads
 *   bit 2        the vertical passes with a strip's rows in registers (stm_k_pq_v12r / stm_k_pq_v12q; 0: stm_k_pq_v12t)
 *   bit 3        the last horizontal pass + WTA on the register ring (stm_k_pq_hsr; 0: an LDS walk, or a volume is kept)
 *   bits 8..15   waves per block of the cost-fusing streaming first pass stm_k_pq_hc: 12 (192-pixel segments), 8 (128-pixel
 *                segments), or 0 when another kernel runs the first pass
 *   bit 16       that pass splits an image row over more than one block
 * Bits 8..16 describe the plan of stm_k_pq_hc: what runs under stm_set_agg_variant(2000000), and the plan that stm_k_pq_hc2
 * replaces where stm_first_pass_path is not 0 (the other bits hold for both).
 * An addition: the reference has one aggregation path and no such query. */
int         stm_agg_path(int num_disp, int zero_disp, int num_rows, int num_cols, int usd, int stages);
/* Whether such a frame call runs its first horizontal pass on stm_k_pq_hc2 -- one block sweeps a part of an image row for BOTH views
 * from one ring of initial costs, each cost evaluated once -- under the current stm_set_agg_variant: the blocks (parts) per image
 * row of that kernel, or 0 when stm_k_pq_hc or another kernel runs the pass.  It runs where stm_agg_path reports bit 1 and 12 waves,
 * 0 <= zero_disp < num_disp, and not under variant 2000000.  Host arithmetic only, from the dispatcher's own functions, like
 * stm_agg_path.  An addition. */
int         stm_first_pass_path(int num_disp, int zero_disp, int num_rows, int num_cols, int usd, int stages);
/* The order of the 64 hypotheses inside a pixel's 256-byte record of the pixel-major volumes of such a frame call under the current
 * stm_set_agg_variant, as the last horizontal pass finds it: -1 where stm_agg_path does not report bit 1; 0 = hypothesis d at float d
 * in both volumes, written as sixteen 4-byte stores per tile of 16 pixels or rows (variant 2000000000); 2 (the default) = the first
 * pass and the vertical kernel each write float 16 b + n of their registers at float 4 n + b, as four 16-byte stores per tile, which
 * leaves hypothesis 4 n + b at float 16 b + n of the volume the last pass reads (1, that permutation applied once, is the first
 * volume's order and never the answer).  The order is internal to the three aggregation kernels: the maps are the same either way.
 * Host arithmetic only, from the dispatcher's own functions, like stm_agg_path.  An addition. */
int         stm_px_order(int num_disp, int zero_disp, int num_rows, int num_cols, int usd, int stages);
/* Test access to the aggregation chain of the calling thread's frame calls.  All four null = off (the default).  An addition.
 * Every buffer is the caller's device memory, float [2][num_disp][H][W]: view 0 is the left and 1 the right, the true hypothesis d
 * ascends, only d < num_disp is stored, and H x W is the size the pair is matched at (the match size of the _2* calls).  While a
 * pointer is set, every frame entry of the thread (stm_adcensus_stm, stm_d_adcensus_stm, _t, _nv12, _2 ..) does this on the frame's
 * stream, each copy as a launch directly behind the pass that produced the volume:
 *   d_h1         receives the volume after the first horizontal pass;
 *   d_v2         receives the volume after both vertical passes;
 *   d_inject_v2  is then written over the chain's V2 volumes, before the last horizontal pass reads them (with stage bit 0x200 the
 *                sub-pixel step reads the injected volume as well).  The padding hypotheses d >= num_disp of the volumes' last chunk
 *                take -1.0f: every last pass guards d >= num_disp itself, so a broken guard shows as a winner outside the range;
 *   d_h4         receives the last pass's output, but only where the chain keeps it (stage bit 0x100 on the matrix pipe; the
 *                vector-ALU chains never write it, and a vector-ALU frame with 0x100 aggregates through the per-stage kernels
 *                and is not tapped at all).
 * The copy kernels know the chain's layouts (PQ, pixel-major in each hypothesis order, quads); no aggregation kernel knows of the tap,
 * no workspace is taken, and stm_agg_path, stm_first_pass_path and stm_px_order answer the same with the tap on and off.  With the tap
 * off there is no extra launch.  Per host thread, read when a call enqueues its kernels; the frames of a stream
 * (stm_stream_submit) never see it.  The per-stage stm_ca_cross / stm_d_ca_cross is not tapped.  Returns 0, or -1 with stm_last_error
 * set and the tap unchanged for a pointer that is not 4-byte aligned (an error like any other: the default error mode exits). */
int         stm_set_agg_tap(float *d_h1, float *d_v2, float *d_h4, const float *d_inject_v2);
/* dr_irv / d_dr_irv / the frame calls: 0 (default) = the reference's accept rule, (winning bin index + zero_disp) / S > thresh_h
 * (d_dr_irv.cu:36 -- the bin INDEX, SURVEY A-Q17 iv); 1 = the paper's rule, (winning bin's COUNT) / S > thresh_h (Mei et al.,
 * region voting).  An addition: the reference has no such switch. */
void        stm_set_irv_paper_ratio(int on);
/* Region voting over column runs (stm_k_irv_vote_cm) gives a wave `entries` consecutive entries of the outlier list, and from the
 * second one on it updates the histogram of the region before instead of counting the region anew.  0 (the default) = the
 * kernel's own rule, max(1, min(16, listed outliers >> 14)), under which a view with fewer than 32768 listed outliers never takes
 * the update; 1 .. 16 = that many, whatever the list's length (the tests' way to the update at small sizes; results do not
 * depend on it).  Read when a call enqueues its kernels, like stm_set_irv_paper_ratio.  Returns 0; a refused value is an error like
 * any other: under stm_set_error_mode(1) the call returns -1 with stm_last_error set and the setting unchanged, under the default
 * mode 0 the process exits.  An addition: the reference has no such kernel. */
int         stm_set_irv_chunk(int entries);
/* Which region-voting kernels a call takes for these arguments under the current stm_set_agg_variant, stm_set_irv_paper_ratio and
 * stm_set_irv_chunk.  Host arithmetic only: nothing is launched, no device is touched, no argument is screened, and the answer
 * comes from the very function the calls dispatch through.  device_flavour: 1 = stm_d_dr_irv and the frame calls, 0 = stm_dr_irv
 * (one vote); with_dcc: 1 = a frame call (both views, the L/R check in front, arms of its own making), 0 = the per-stage calls
 * (the caller's arm table).  A bit field:
 *   bit 0        pruning: outliers that can never be accepted are not listed (stm_k_irv_rowcount + stm_k_irv_colprefix, or the chain)
 *   bit 1        column runs (stm_k_irv_compact_cm, stm_k_irv_vote_cm; 0: the raster list, stm_k_irv_compact, stm_k_irv_vote)
 *   bit 2        the frame's short chain (stm_k_dcc_irv_rows + stm_k_irv_compact_cm<true>)
 *   bits 8..11   log2 of the edge of the tiles in which accepted pixels are recorded between iterations
 *   bits 16..20  the forced entries per trip where column runs vote, else 0
 * An addition: the reference has one path and no such query. */
int         stm_irv_path(int num_rows, int num_cols, int usd, int iterations, int device_flavour, int with_dcc);
/* The calling thread's display geometry (see stm_mux_multiview_lens for the definition and the argument rules); the default is
 * mode 0.  With mode != 0 every frame call that renders -- stm_adcensus_stm, stm_d_adcensus_stm, _t, _nv12, and _2 / _2s in both
 * flavours -- interlaces through that definition instead of the reference's formula; `angle` is then ignored and not screened.
 * With mode 0 not one launch or argument changes.  Modes 1 and 2 follow stm_set_agg_variant(200) into the un-fused form (every
 * view written, then interlaced); mode 3 has no views, so it always takes the fused kernel.  This is an output geometry, not a
 * stage: no `stages` bit belongs to it.  Returns 0, or -1 with stm_last_error set and the thread's geometry unchanged. */
int         stm_set_lens(int mode, double pitch, double slope, double centre);
/* The calling thread's depth budget (an addition: the reference's N views always span exactly the camera baseline -- view v sits at
 * shift = 1 - v/(N-1) -- and the zero-parallax plane is wherever zero_disp put it).  A lenticular panel has a limited usable
 * parallax range; a scene that exceeds it ghosts.  mode 0 = off (the default: not one launch, argument or kernel of the path
 * changes), 1 = manual (gain, conv), 2 = automatic (gain and conv fitted to each frame's disparity range on the device, see
 * stm_set_depth_auto and stm_depth_fit).  With mode != 0 every frame call that renders -- stm_adcensus_stm, stm_d_adcensus_stm, _t,
 * _nv12, and _2 / _2s in both flavours -- takes every sample by the rule below.  It combines with every lens mode and with 0x800.
 * There are no views to write, so the fused renderer is taken always, also under stm_set_agg_variant(200).  Like the lens geometry
 * this is an output geometry, not a stage: no `stages` bit belongs to it.
 *
 * Sign convention: the maps hold delta = x_right - x_left (disp = d - zero_disp).
 * Sample rule.  A sample is taken for the view position s: for a discrete view v, s = (float)(1 - v/(N-1)) as the reference
 * evaluates it (d_io.cu:189); in lens mode 3, the sub-pixel's own shift.  (xs, ys) is the interlacer's sampling position; gain and
 * conv are floats, conv in input-view pixels.  f32 or f64 as written, one operation per line, no contraction, C fminf / fmaxf:
 *   t   = (double)s - 0.5
 *   u   = (double)gain * t
 *   s2  = (float)(0.5 + u)
 *   u   = (double)conv * t
 *   off = (float)u
 *   cx  = xs + off
 *   cx  = fminf(fmaxf(cx, 0), (float)(Win - 1))
 * The value is fast_bilinear_interp's combination (d_mux_multiview.cu:10-36) of the <= 4 neighbours of (cx, ys), each neighbour
 * being the renderer's general form at shift s2: shift_l = -s2, shift_r = (float)(1.0 - (double)s2), both backward warps
 * (truncating, or linear with 0x800), masks, blend, u8 wrap.  The end-view shortcut (view 0 = the right image, view N-1 = the left
 * image) is not taken; a neighbour of weight exactly 0 is not evaluated.  Lens mode 2 blends two views, each with its own s2 and cx.
 * A scene point of disparity delta is then shown with the end-to-end disparity gain * delta - conv.  gain > 1 makes s2 leave [0, 1]:
 * the formulas are used unchanged, which is extrapolation beyond the two cameras, with the quality that implies (disocclusions the
 * masks were not made for).  gain = 1, conv = 0 renders the interior views 1 .. N-2 as mode 0 does and the two end views as warps
 * at s = 1 and s = 0 instead of the unwarped images.
 * Argument rules: mode 0, 1 or 2; in mode 1 gain finite in [0, 8], conv finite with |conv| <= 4096 (both ignored otherwise); mode 2
 * needs a budget from stm_set_depth_auto first.  Returns 0, or -1 with stm_last_error set and the thread's setting unchanged. */
int         stm_set_depth(int mode, float gain, float conv);
/* Mode 2's parameters (kept when the mode changes): the budget [disp_lo, disp_hi] of end-to-end disparity in input-view pixels
 * (disp_lo < disp_hi, both finite and of magnitude <= 4096), max_gain in (0, 8] (1 = never amplify), clip_permille in 0 .. 499 (the
 * share of pixels ignored at either end of the range; a sequence's default is 20), rate in (0, 1] (1 = every frame on its own),
 * d_state = four floats in device memory, {valid, gain, conv, 0}, or null.  In mode 2 the frame call runs stm_d_depth_fit on the
 * maps it renders from (the up-scaled maps of the reduced frame, the stabilised maps of 0x2000) with these parameters and d_state,
 * and the renderer of the same frame reads gain and conv from that memory: nothing is synchronised or read back.  A null d_state
 * means scratch memory, with every frame fitted on its own.  A caller resets the history, for a scene cut, by zeroing `valid` (stm_set_cut does it on the device).
 * Returns 0, or -1 with stm_last_error set and the old parameters in place. */
int         stm_set_depth_auto(float disp_lo, float disp_hi, float max_gain, int clip_permille, float rate, float *d_state);
/* The calling thread's view antialiasing (an addition; stm_view_prefilter has the definition and the reason).  The depth budget above
 * flattens a scene that exceeds the panel's range; this is the second remedy, band-limiting what stays off the screen plane.
 * mode 0 = off (the default; the other arguments are ignored, and not one launch, argument or kernel of any call changes), 1 = on:
 * every frame call that renders -- stm_adcensus_stm, stm_d_adcensus_stm, _t, _nv12, and _2 / _2s / _2t / _2nv12 in both flavours where
 * they exist -- filters the left image by disp_l and the right image by disp_r, exactly as stm_d_view_prefilter would with the call's
 * num_views, into fresh workspace, before it renders; whichever renderer the frame takes (the fused interlacer, every lens mode, the
 * depth renderers, both quilt kernels with BGR or NV12 output, the un-fused forms of stm_set_agg_variant(200), whose end views are then
 * the filtered images) is handed the filtered pair.  gain and conv: depth mode 0 filters with gain 1, conv 0; mode 1 with the setting;
 * mode 2 with the state -- the fit runs first and the prefilter reads gain and conv on the device where the renderers read them.
 * The unfiltered images (0x2000's history, _nv12's d_img_l / d_img_r) and the maps never change; an overlay is composited afterwards
 * and is not blurred.  It is an output quality setting, not a stage: no `stages` bit belongs to it, and a frame call whose `stages`
 * low byte is below 3 renders nothing and ignores it.
 * Argument rules: mode 0 or 1; with mode 1 stm_view_prefilter's rules for strength, max_radius and gate.  Returns 0, or -1 with
 * stm_last_error set and the thread's setting unchanged. */
int         stm_set_antialias(int mode, float strength, int max_radius, float gate);
/* out_mode = {mode, max_radius}, out = {strength, gate} as the last accepted stm_set_antialias left them ((0, 0) and (0, 0) if none
 * was made, and after mode 0).  A frame stream's own setting is not visible here except during its submit. */
void        stm_get_antialias(int out_mode[2], float out[2]);
/* The calling thread's vertical alignment of the pair (an addition: the reference takes rectified studio masters, and every matcher
 * here searches along image rows.  A pitch, roll or focal-length difference between two lenses leaves a vertical offset between the
 * eyes that is constant, linear across the width, or linear down the height; a few pixels of it send AD-Census to the wrong
 * disparity on every horizontal edge).  mode 0 = off (the default: not one launch, argument or kernel of any call changes),
 * 1 = manual (the field a, b, c), 2 = automatic (the field measured on every frame on the device: stm_set_align_auto, stm_align_fit).
 * The field is dy(x, y) = a + b u + c v with u = x - (W-1)/2, v = y - (H-1)/2 on one unpacked eye of H x W pixels; the left eye is the
 * reference, and the aligned right eye at (y, x) is the right eye sampled at row y + dy(x, y) by stm_align_rows' rule.
 * With mode != 0 the frame calls stm_d_adcensus_stm, _t, _nv12, _2s, _2t, _2nv12 (and the host flavours through them) first write the
 * aligned, unpacked, converted pair as one side-by-side BGR frame into the workspace (one launch; mode 2: three small launches before
 * it for the measurement, always on the full-resolution input) and then ARE the plain BGR frame call on that frame, packing off:
 * every `stages` bit, the reduced-resolution frame, and the lens, depth, layout, output, overlay and antialias settings behave as they
 * do on a side-by-side BGR frame; _nv12's d_img_l / d_img_r receive the aligned images.  With 0x2000 on a BGR frame (_t, _2t) the
 * previous frame passes through the same kernel with the CURRENT frame's field (one more launch), so both frames are compared in
 * one geometry.  With 0x2000 on an NV12 frame the history is the caller's d_prev_img_l / d_prev_img_r as the previous call wrote
 * them: aligned by that frame's field.  Rules under mode != 0: an unpacked BGR frame needs num_cols_sbs >= 2 * num_cols; mode 2
 * needs num_rows >= 4, num_cols >= 8 and (num_rows/4 + 1) * (num_cols/8 + 1) <= 8421504 (any frame up to 16384 x 16384).
 * Argument rules: mode 0, 1 or 2; in mode 1 a, b, c finite (ignored otherwise; the offset itself is clamped to +-64 rows per pixel).
 * Returns 0, or -1 with stm_last_error set and the thread's setting unchanged. */
int         stm_set_align(int mode, float a, float b, float c);
/* Mode 2's parameters (kept when the mode changes; the defaults are 16, 1, null): radius in 1 .. 32, the search range in rows; rate
 * in (0, 1] (1 = every frame on its own); d_state = four floats in device memory, {valid, a, b, c}, or null.  In mode 2 the frame
 * call runs stm_d_align_fit's measurement on its input with these parameters and d_state, and the kernel that applies the field
 * reads a, b, c from that memory: nothing is synchronised or read back.  A null d_state means scratch memory, with every frame
 * fitted on its own.  A caller resets the history, for a scene cut, by zeroing `valid` (stm_set_cut does it on the device).  Returns 0, or -1 with stm_last_error set
 * and the old parameters in place. */
int         stm_set_align_auto(int radius, float rate, float *d_state);
/* out_mode = {mode, radius}, out = {a, b, c, rate} as the last accepted calls left them.  A frame stream's own setting is not
 * visible here except during its submit. */
void        stm_get_align(int out_mode[2], float out[4]);
/* The calling thread's colour balance between the eyes (an addition: the reference takes graded studio masters.  Two-lens phones and
 * hand-built rigs have two sensors with different exposure, white balance and tone curves, while the AD half of AD-Census is an
 * absolute colour difference, the cross arms are built from colour thresholds, and every rendered view blends the two images).
 * Three per-channel 256-entry tables are applied to the RIGHT eye ahead of the matcher; the left eye is the reference, as with
 * stm_set_align.  mode 0 = off (the default: not one launch, argument or kernel of any call changes), 1 = given (lut768: B, G, R,
 * 256 bytes each, copied; no monotonicity demanded), 2 = measured (lut768 ignored; the tables fitted on every frame on the device
 * from the two eyes' histograms: stm_set_balance_auto, stm_balance_fit).
 * With mode != 0 the frame calls stm_d_adcensus_stm, _t, _nv12, _2s, _2t, _2nv12 (and the host flavours through them) first write
 * the unpacked, converted pair, its right eye through the tables, as one side-by-side BGR frame into the workspace (one launch;
 * mode 2: three small launches before it for the measurement) and then ARE the plain BGR frame call on that frame, packing off,
 * exactly as under stm_set_align.  With an alignment set as well the balance comes second and measures the aligned pair: two passes
 * over the pair.  With 0x2000 on a BGR frame the previous frame passes through the same kernel with the CURRENT frame's tables;
 * on an NV12 frame the history is what the previous call handed out.  Rules under mode != 0: an unpacked BGR frame needs
 * num_cols_sbs >= 2 * num_cols; mode 2 needs num_rows * num_cols < 2^31.
 * Returns 0, or -1 with stm_last_error set and the thread's setting unchanged (mode not 0, 1, 2; mode 1 with a null lut768). */
int         stm_set_balance(int mode, const unsigned char *lut768);
/* Mode 2's parameters (kept when the mode changes; the defaults are 48, 1, null): max_shift in 0 .. 255, the most levels a table
 * moves a level by; rate in (0, 1] (1 = every frame on its own; NaN is refused); d_state = 769 ints in device memory, {valid, 768
 * levels in 1/256 units}, or null.  In mode 2 the frame call runs stm_d_balance_fit's measurement on its input with these
 * parameters and d_state, and the kernel that applies the tables reads them from that memory: nothing is synchronised or read
 * back.  A null d_state means scratch memory, with every frame fitted on its own.  A caller resets the history, for a scene cut,
 * by zeroing `valid` (stm_set_cut does it on the device).  Returns 0, or -1 with stm_last_error set and the old parameters in place. */
int         stm_set_balance_auto(int max_shift, float rate, int *d_state);
/* out_mode = {mode, max_shift}, *out_rate and out_lut (mode 1's tables; the identity otherwise) as the last accepted calls left
 * them.  A frame stream's own setting is not visible here except during its submit. */
void        stm_get_balance(int out_mode[2], float *out_rate, unsigned char out_lut[768]);
/* The calling thread's shot-change detector (an addition: the reference keeps nothing from frame to frame.  The three recursive
 * states above -- stm_set_depth_auto's, stm_set_align_auto's, stm_set_balance_auto's -- follow a sequence at a `rate`, and with any
 * rate < 1 the first frames of a new shot would be conditioned by the previous shot's numbers).  mode 0 = off (the default: the
 * other arguments are ignored, and not one launch, argument or kernel of any call changes), 1 = on: d_state = 260 ints in device
 * memory, {valid, cut, since, score, sig[256]} (stm_cut_detect), the caller's, zeroed at the start; null is refused, since without
 * history there is nothing to detect.
 * With mode 1 the frame calls stm_d_adcensus_stm, _t, _nv12, _2s, _2t, _2nv12 (and the host flavours through them) first run
 * stm_d_cut_detect's three launches on the left eye of their full-resolution input, read straight from the frame (BGR or NV12, any
 * packing), ahead of the alignment's measurement.  The reset pointers are the d_state of depth mode 2 (where the call renders),
 * alignment mode 2 and balance mode 2, each only where that mode is in force for the call and the pointer is not null (a null one
 * means scratch memory and has no history to lose).  On a cut their `valid` words are zero before their fits run, so each fit starts
 * afresh on that frame; nothing is synchronised or read back.  The caller reads the flag from d_state[1] when it likes (an encoder
 * behind stm_set_output places a key frame there).  0x2000 is untouched: its colour gate already refuses to blend across a cut.
 * Rules under mode 1: num_rows, num_cols >= 4 and num_rows * num_cols < 2^31 in every frame call.
 * Known limits: dissolves and fades are not cuts (the recursive filters follow them as they follow anything gradual); a global
 * exposure step of about 16 levels can score as a cut, and a false cut costs one frame fitted on its own.
 * Returns 0, or -1 with stm_last_error set and the thread's setting unchanged (mode not 0 or 1; in mode 1 thresh_permille outside
 * 1 .. 1000, min_gap outside 1 .. 2^20, a null d_state). */
int         stm_set_cut(int mode, int thresh_permille, int min_gap, int *d_state);
/* out = {mode, thresh_permille, min_gap} as the last accepted calls left them (before any: 0, 370, 1).  A frame stream's own
 * setting is not visible here except during its submit. */
void        stm_get_cut(int out[3]);
/* The calling thread's active picture area (an addition: the reference matches and measures black bars as if they were picture.  A
 * 2.39:1 film in a 16:9 frame has a quarter of its pixels in two bars, where the matcher has nothing to match: pure black ties at
 * -zero_disp, codec noise matches anywhere, and both go straight into depth mode 2's range and into the "nearest content" under a
 * subtitle that lies in the bottom bar).  mode 0 = off (the default: the other arguments are ignored, and not one launch, argument or
 * kernel of any call changes), 1 = a given rectangle rect = {top, bottom, left, right}: rows [top, bottom), columns [left, right) of
 * one unpacked eye, 2 = measured: every frame call runs stm_d_active_detect's three launches on the left eye of its full-resolution
 * input as given (BGR or NV12, any packing), after the shot-change detector and before the alignment's measurement -- the left eye is
 * the reference of the alignment and the balance, so the result depends on neither -- with stm_set_active_auto's parameters and
 * state, restart = 0 (1 with a null state) and, where stm_set_cut is on, its state.
 * With mode != 0 the frame calls stm_d_adcensus_stm, _t, _nv12, _2s, _2t, _2nv12 (and the host flavours through them):
 *   - fit depth mode 2 as stm_d_depth_fit_rect does, under the rectangle read on the device;
 *   - fit the automatic overlay placement (stm_set_overlay_auto) as stm_d_overlay_fit_rect does;
 *   - with fill = 1, run stm_d_active_fill(., fill_disp) on both maps they hand back, after the temporal step and before the
 *     renderer, whatever the `stages` low byte is, in the reduced-resolution calls on the up-scaled maps: the maps come back clean
 *     and side bars render as one stable surface.
 * Nothing is synchronised or read back.  Rules under mode 1: 0 <= top < bottom <= num_rows and 0 <= left < right <= num_cols in every
 * frame call; under mode 2: num_rows * num_cols < 2^31.  A frame call that breaks one is refused through stm_last_error before
 * anything is launched or written.
 * Not treated: the cut signature, the alignment's profiles and the balance's histograms keep reading the whole frame; the bars of
 * the finished frame are not painted (every warp is along a row, so bar rows sample bar rows); bars that differ between the eyes
 * (floating windows).
 * Argument rules: mode 0, 1 or 2; in mode 1 a non-null rect with 0 <= top < bottom and 0 <= left < right; with mode != 0 fill 0 or 1
 * and fill_disp finite with |fill_disp| <= 4096.  Returns 0, or -1 with stm_last_error set and the thread's setting unchanged. */
int         stm_set_active(int mode, const int rect[4], int fill, float fill_disp);
/* Mode 2's parameters, kept when the mode changes: thresh_luma 0 .. 254 (default 24: limited-range black, 16, plus noise),
 * lit_permille 0 .. 999 (10), max_bar_permille 0 .. 450 (300), hold 1 .. 2^20 (12); stm_active_detect has the definition.  d_state =
 * 16 ints in device memory the caller owns, zeroes once and keeps alive while the setting is on, or null: scratch memory, every frame
 * measured on its own.  Returns 0, or -1 with stm_last_error set and the old parameters in place. */
int         stm_set_active_auto(int thresh_luma, int lit_permille, int max_bar_permille, int hold, int *d_state);
/* out = {mode, top, bottom, left, right, fill, thresh_luma, lit_permille, max_bar_permille, hold}, *fill_disp the fill value, as the
 * last accepted calls left them (before any: 0, 0, 0, 0, 0, 0, 24, 10, 300, 12 and 0).  A frame stream's own setting is not visible here
 * except during its submit. */
void        stm_get_active(int out[10], float *fill_disp);
/* The calling thread's output geometry (an addition: the reference shows its views in one form only, sub-pixel interlaced).
 * layout 0 = the interlaced frame (the default; tiles_x, tiles_y, order and filter are ignored, and not one launch, argument or
 * kernel changes), 1 = a quilt: the views side by side as a grid of tiles, whole, for a display that interlaces with its own
 * calibration, for an encoder of multiview video, or to get a depth-retargeted stereo pair back (num_views 2, tiles 2 x 1, order 2,
 * stm_set_depth).  With layout 1 every frame call that renders -- stm_adcensus_stm, stm_d_adcensus_stm, _t, _nv12, and _2 / _2s in
 * both flavours -- writes the quilt defined at stm_quilt_multiview into its output frame; `angle` is then ignored and not screened.
 * The views V(v, x, y, c) are the renderer's, none is written to memory:
 *   depth mode 0      view 0 = the right image, view N-1 = the left image, view v the reference's d_dibr_dbm at
 *                     shift = (float)(1 - v/(N-1)) (d_io.cu:189)
 *   depth mode 1, 2   stm_set_depth's sample rule at s = (float)(1 - v/(N-1)), xs = (float)x, ys = (float)y (so wy = 0 and only row
 *                     y is read), the conv offset included; mode 2 reads gain and conv on the device as in the interlaced frame
 * with the linear tap under 0x800 in both.  Under filter 0 the sample at a fractional (xs, ys) is the renderer's own: the
 * four-neighbour combination of view v's samples in depth mode 0, stm_set_depth's sample rule at (xs, ys) in modes 1 and 2.
 * Depth mode 0 follows stm_set_agg_variant(200) into the un-fused form (every view written, then stm_d_quilt_multiview); with a depth
 * budget there are no views to write and the fused kernels are taken always.
 * Errors of a frame call under layout 1, through stm_last_error before anything is launched or written: tiles_x * tiles_y !=
 * num_views; a tile of width num_cols_out / tiles_x == 0 or height num_rows_out / tiles_y == 0; a lens mode != 0 on the thread (a quilt
 * is not interlaced).  A frame call whose `stages` low byte is below 3 renders nothing and ignores the layout, as it ignores the lens.
 * This is an output geometry, not a stage: no `stages` bit belongs to it.
 * Argument rules: layout 0 or 1; with layout 1 tiles_x, tiles_y in 1 .. 65535, order in 0 .. 3, filter 0 or 1.  Returns 0, or -1 with
 * stm_last_error set and the thread's layout unchanged. */
int         stm_set_layout(int layout, int tiles_x, int tiles_y, int order, int filter);
/* out[0 .. 4] = the calling thread's layout, tiles_x, tiles_y, order and filter as the last accepted stm_set_layout left them
 * ((0, 1, 1, 0, 0) if none was made, and after layout 0).  A frame stream's own layout is not visible here except during its submit. */
void        stm_get_layout(int *out);
/* The calling thread's output format (an addition: the reference writes BGR only, which no hardware video encoder takes).
 * format 0 = BGR, elem_sz bytes a pixel (the default; matrix, pitch and uv_row are ignored, and not one launch, argument or kernel
 * changes), 1 = NV12.  With format 1 the d_interlaced / interlaced argument of every frame call that renders -- stm_adcensus_stm,
 * stm_d_adcensus_stm, _t, _nv12, and _2 / _2s / _2t / _2nv12 in both flavours where they exist -- is ONE NV12 surface holding the
 * picture that stm_mux_nv12 (the definition and the matrices are there) gives on the BGR quilt the call would have written:
 *   Y plane    num_rows_out rows of P bytes from byte 0;              P = pitch, or num_cols_out if pitch == 0
 *   UV plane   num_rows_out / 2 rows of P bytes from byte P * R;      R = uv_row, or num_rows_out if uv_row == 0
 * so an encoder's pitch and height alignment are met in place.  elem_sz keeps describing the input pixels only.  The conversion runs
 * inside the kernel that renders the pixels: no BGR quilt is written (stm_set_agg_variant(200) with depth mode 0 is the un-fused
 * form: the BGR quilt in the workspace, then stm_d_mux_nv12's kernel).  The device flavours leave every byte of the surface that is
 * neither a Y nor a UV sample as it was; the host flavours return those bytes 0 and copy P * (R + num_rows_out / 2) bytes.
 * Errors of a frame call under format 1, through stm_last_error before anything is launched or written: the thread's layout is 0
 * (chroma subsampling destroys a sub-pixel interlaced frame: NV12 exists for quilts only); num_rows_out or num_cols_out odd; a tile
 * width num_cols_out / tiles_x or height num_rows_out / tiles_y odd (every tile starts on a chroma sample, so no chroma sample mixes
 * two views, and the remainders are then even too); P < num_cols_out; R < num_rows_out.  (P * (R + num_rows_out / 2) fits 63 bits for
 * every int P, R and num_rows_out, so that rule needs no test.)  A frame call whose `stages` low byte is below 3 renders nothing and
 * ignores the format, as it ignores the layout.
 * Argument rules: format 0 or 1; with format 1 matrix in 0 .. 3, pitch >= 0, uv_row >= 0.  Returns 0, or -1 with stm_last_error set
 * and the thread's format unchanged. */
int         stm_set_output(int format, int matrix, int pitch, int uv_row);
/* out[0 .. 3] = the calling thread's format, matrix, pitch and uv_row as the last accepted stm_set_output left them ((0, 0, 0, 0) if
 * none was made, and after format 0).  A frame stream's own format is not visible here except during its submit. */
void        stm_get_output(int out[4]);
/* The calling thread's overlay (an addition; stm_mux_overlay has the definition): subtitles, a logo or a player's OSD composited
 * into every finished frame at a chosen depth.  mode 0 = off (the default; the other arguments are ignored, and not one launch,
 * argument or kernel of any frame call changes), 1 = on: every frame call that renders -- stm_adcensus_stm, stm_d_adcensus_stm, _t,
 * _nv12, and _2 / _2s / _2t / _2nv12 in both flavours where they exist -- composites the overlay as its LAST launch, exactly as
 * stm_d_mux_overlay would on the frame it wrote, under the thread's lens (stm_set_lens) and layout (stm_set_layout), with the call's
 * num_views, angle, num_rows_out, num_cols_out and elem_sz.  d_overlay is DEVICE memory in both flavours, ov_rows x ov_cols x 4 bytes,
 * which the caller owns and keeps alive and unchanged while the setting is on, as d_state of stm_set_depth_auto.
 * It is an output addition, not a stage: no `stages` bit belongs to it, a frame call whose `stages` low byte is below 3 renders
 * nothing and ignores it, and the disparity maps never change.
 * Errors of a frame call under mode 1, through stm_last_error before anything is launched or written: the thread's output format is 1
 * (NV12) -- compositing on a chroma-subsampled surface needs a definition of its own, which is out of scope; format 1 with an
 * overlay is refused whichever of the two was set first.
 * Argument rules: mode 0 or 1; with mode 1 stm_mux_overlay's rules for the overlay's own arguments (a non-null, 4-byte aligned
 * pointer, the sizes, the position, the disparity).  Returns 0, or -1 with stm_last_error set and the thread's setting unchanged. */
int         stm_set_overlay(int mode, const unsigned char *d_overlay, int ov_rows, int ov_cols, int x0, int y0, float disparity);
/* out[0 .. 4] = the calling thread's mode, ov_rows, ov_cols, x0 and y0, *disparity its disparity, as the last accepted
 * stm_set_overlay left them ((0, 0, 0, 0, 0) and 0 if none was made, and after mode 0).  A frame stream's overlay is never visible here. */
void        stm_get_overlay(int out[5], float *disparity);
/* The calling thread's automatic overlay placement (an addition; stm_overlay_fit has the definition).  A setting of its own, not a
 * mode of stm_set_overlay: mode 0 (the default) changes nothing anywhere.  While mode 1 is on AND the thread's overlay is on, every
 * rendering frame call, after its renderer, runs stm_d_overlay_fit on the maps the renderer read -- with the thread's overlay, the
 * view of the thread's layout (the output frame, or one tile of a quilt), the depth budget in force ((1, 0) in depth mode 0, the
 * setting in mode 1, the state the same frame's fit left in mode 2, read on the device), restart = 0 and, where stm_set_cut is on,
 * its state -- and then composites as stm_d_mux_overlay would at fminf(fmaxf(state[1], limit_lo), limit_hi) (a NaN: limit_lo), read
 * on the device: nothing is read back, the frame is byte for byte stm_d_mux_overlay's at that disparity.  stm_set_overlay's own
 * disparity is ignored but still screened.  d_state = four floats in device memory {valid, disparity, nearest, 0} the caller owns,
 * zeroes once and keeps alive while the setting is on, or null: four zeroed floats of the workspace, every frame fitted on its own.
 * Mode 0 ignores the other arguments and restores the defaults.  Argument rules as stm_overlay_fit's; a refused call leaves the
 * setting as it was.  Return 0, or -1 with stm_last_error set.  stm_get_overlay_auto: out_mode = {mode, near_permille, pad},
 * out = {margin, limit_lo, limit_hi, rate_near, rate_far}. */
int         stm_set_overlay_auto(int mode, int near_permille, float margin, int pad, float limit_lo, float limit_hi, float rate_near,
                                 float rate_far, float *d_state);
void        stm_get_overlay_auto(int out_mode[3], float out[5]);
/* (tests, tools) the bytes of LDS a workgroup of the area filter's staged kernel may take: the block of output pixels it owns is sized
 * so that its footprint's staging fits, and where not even one output pixel's does the per-pixel form runs -- same arithmetic, same
 * bytes.  <= 0: the default, 32768 (five workgroups on a CU); at most 65536.  Process-wide, like stm_set_agg_variant. */
void        stm_set_quilt_lds_limit(int bytes);
/* The calling thread's input packing (an addition; see stm_demux_packed for the definition and the rules): where the two eyes lie in
 * the frame that stm_d_adcensus_stm, stm_d_adcensus_stm_t and stm_d_adcensus_stm_nv12 are given.  The default is (0, 0, 0, 0), the
 * reference's layout, with which not one launch, argument or kernel changes.  Under any other setting num_rows and num_cols stay the
 * size of an eye AFTER unpacking (what every later stage sees), num_cols_sbs stays the frame's row length in pixels, the frame has
 * rows_f rows, and the geometry rules of stm_demux_packed (stm_demux_nv12_packed for the NV12 call) replace num_cols_sbs >= 2 *
 * num_cols; a violation fails through stm_last_error before anything is launched.  The frame is by definition the same call, packing
 * off, on the side-by-side frame whose halves are the two unpacked eyes; the frame's first kernel gathers, filters and (NV12)
 * converts as it fetches, no unpacked frame is materialised, every `stages` bit keeps its meaning and every later kernel is unchanged.
 * With 0x2000, stm_d_adcensus_stm_t's d_prev_img_sbs is the previous PACKED frame and its images are by definition its unpacking
 * (one extra launch); stm_d_adcensus_stm_nv12 takes split history as always.  This is an input geometry, not a stage: no `stages`
 * bit belongs to it.  The host-flavour stm_adcensus_stm and the four adcensus_stm_2 / _2s calls take the reference's layout only:
 * with a packing set on the thread they fail through stm_last_error, they do not ignore it.
 * Returns 0, or -1 with stm_last_error set and the thread's packing unchanged (a setting outside its range; filter != 0 with packing
 * 0 or 2). */
int         stm_set_packing(int packing, int swap, int filter, int gap);
/* out[0 .. 3] = the calling thread's packing, swap, filter and gap as the last accepted stm_set_packing left them ((0, 0, 0, 0) if
 * none was made).  A frame stream's own packing is not visible here except during its submit. */
void        stm_get_packing(int *out);
/* ci_adcensus / d_ci_adcensus (the per-stage calls; the frame calls always compute the clean costs): 0 (default) = clean
 * clamped indexing, the canonical form (SURVEY A-Q7); 1 = reproduce the reference's shared-tile strays at d = 0 in columns
 * 160 k (left cost) and 160 k + 159 (right cost): the census term always, the AD term when num_disp - zero_disp <= zero_disp
 * (d_ci_adcensus.cu:57-59,117-120; d_ci_census.cu:240-246; d_ci_ad.cu:133-144).  Meaningful for num_cols % 160 == 0, the
 * only widths for which the reference's own launch fills its tiles.  An addition: the reference has no such switch. */
void        stm_set_ref_quirks(int on);

/* ------------------------------------------------------- cost init (a1-a7) */
/* d_ci_adcensus.h:23-25  ci_adcensus  (d_ci_adcensus.cu:188-378) */
void stm_ci_adcensus(unsigned char *img_l, unsigned char *img_r, float **cost_l, float **cost_r,
                     float ad_coeff, float census_coeff, int num_disp, int zero_disp,
                     int num_rows, int num_cols, int elem_sz);
/* d_ci_adcensus.h:16-21  d_ci_adcensus (d_ci_adcensus.cu:38-186).  Fills the host and device plane
 * tables exactly as :150-157 does: L plane d at memory + d*H*W, R plane d at memory + (D + d)*H*W. */
void stm_d_ci_adcensus(unsigned char *d_img_l, unsigned char *d_img_r,
                       float **d_adcensus_cost_l, float **d_adcensus_cost_r,
                       float **h_adcensus_cost_l, float **h_adcensus_cost_r,
                       float *d_adcensus_cost_memory,
                       float ad_coeff, float census_coeff, int num_disp, int zero_disp,
                       int num_rows, int num_cols, int elem_sz);

/* ------------------------------------------------ cross aggregation (a8-a12) */
/* d_ca_cross.h:19-21  ca_cross (d_ca_cross.cu:275-444): cost untouched, result in acost, arms in cross */
void stm_ca_cross(unsigned char *img, unsigned char **cross, float **cost, float **acost,
                  float ucd, float lcd, int usd, int lsd,
                  int num_disp, int num_rows, int num_cols, int elem_sz);
/* d_ca_cross.h:13-17  d_ca_cross (d_ca_cross.cu:174-273): RESULT LANDS IN d_cost (input overwritten),
 * d_acost/d_acost_memory are scratch; h_acost and d_acost tables are filled as :207-210 does. */
void stm_d_ca_cross(unsigned char *d_img, float **d_cost,
                    float **d_acost, float **h_acost, float *d_acost_memory,
                    unsigned char **d_cross,
                    float ucd, float lcd, int usd, int lsd,
                    int num_disp, int num_rows, int num_cols, int elem_sz);

/* ------------------------------------------------- disparity selection (a13,a14) */
/* d_dc_wta.h:16-18 / :12-14  (d_dc_wta.cu:9-59) */
void stm_dc_wta(float **cost, float *disp, int num_disp, int zero_disp, int num_rows, int num_cols);
void stm_d_dc_wta(float **d_cost, float *d_disp, int num_disp, int zero_disp, int num_rows, int num_cols);
/* Sub-pixel disparity enhancement (Mei et al. section 3.4, last step; an addition: the reference has none).  cost = the
 * AGGREGATED volume (ca_cross's result, what dc_wta minimises), same pointer contract as dc_wta; disp is refined in place.
 * A pixel is eligible when v = disp[p] is a whole number with 1 <= d = v + zero_disp <= num_disp - 2 and cm = cost[d-1][p],
 * c0 = cost[d][p], cp = cost[d+1][p] are finite; then, each step one f32 operation in this order:
 *   den = (cm + cp) - (c0 + c0);  if den > 0:  disp[p] = v + min(max((cm - cp) / (den + den), -0.5), 0.5)
 * (correctly rounded division).  Every other pixel keeps its value.  Parity is against a numpy statement of these lines on the
 * oracle's volumes (parity unpinned by nature, as for HSLO: the reference has no such step). */
void stm_dc_subpixel(float **cost, float *disp, int num_disp, int zero_disp, int num_rows, int num_cols);
void stm_d_dc_subpixel(float **d_cost, float *d_disp, int num_disp, int zero_disp, int num_rows, int num_cols);
/* d_dc_hslo.h:18-22  dc_hslo (d_dc_hslo.cu:97-221, a stub in the reference; implemented here, parity unpinned) */
void stm_dc_hslo(float **cost, float *disp, unsigned char *img_l, unsigned char *img_r,
                 float T, float H1, float H2, int num_disp, int zero_disp,
                 int num_rows, int num_cols, int elem_sz);
/* device flavour: the reference has none; same contract as the other d_ calls */
void stm_d_dc_hslo(float **d_cost, float *d_disp, unsigned char *d_img_l, unsigned char *d_img_r,
                   float T, float H1, float H2, int num_disp, int zero_disp,
                   int num_rows, int num_cols, int elem_sz);

/* -------------------------------------------------------- refinement (a15-a17) */
/* MAP VALUES A STAGE CANNOT PLACE.  dr_dcc, dr_irv, filter_bilateral_1, filter_median, dibr_occl and dibr_dfm take whatever map
 * the caller has: NaN, +-inf, values far outside the row.  The reference converts with a plain (int), which is undefined there;
 * these rules define it (host and d_ flavour alike, tests/test_gpu_map_edges.py):
 *   f2i_sat(v)   every float -> int conversion of a map value: truncate toward zero, saturate at INT_MIN / INT_MAX, NaN -> 0
 *                (what v_cvt_i32_f32 does, and the reference's hardware conversion);
 *   no integer sum with a converted value as an operand overflows: a target column is clamp((int64)x +- f2i_sat(v), 0, W - 1).
 * For maps with every value in (-2^31 + 65536, 2^31 - 65536) no conversion saturates and no sum leaves 32 bits. */
/* d_dr_dcc.h:17-19 / :13-15  (d_dr_dcc.cu:84-203).  Host flavour zero-fills the outlier maps itself
 * (:166-171); the device flavour expects them zero-filled by the caller (d_io.cu:138-141). */
/*   c_l = clamp(x + f2i_sat(disp_l[x]), 0, W - 1):  outliers_l[x] = |disp_l[x] - disp_r[c_l]| > 1 (false for a NaN difference),
 *                                                  hit_r[c_l] = 0;
 *   c_r = clamp(x - f2i_sat(disp_r[x]), 0, W - 1):  outliers_r[x] = |disp_r[x] - disp_l[c_r]| > 1,  hit_l[c_r] = 0;
 *   both sums without overflow (x - INT_MIN is column W - 1).  An outlier whose pixel was never hit is class 2. */
void stm_dr_dcc(unsigned char *outliers_l, unsigned char *outliers_r, float *disp_l, float *disp_r,
                int num_rows, int num_cols);
void stm_d_dr_dcc(unsigned char *d_outliers_l, unsigned char *d_outliers_r, float *d_disp_l, float *d_disp_r,
                  int num_rows, int num_cols);
/* d_dr_irv.h:15-19 / :8-13  (d_dr_irv.cu:222-364).  Host flavour votes once and applies `iterations`
 * times (:344-353); device flavour repeats vote+apply (:259-265). */
/*   a reliable pixel votes in bin b = f2i_sat(d) + zero_disp when 0 <= b < max(num_disp, 65), taken without overflow; any other
 *     b counts towards the region's size S only;
 *   where no pixel of the region has a bin the winner is f2i_sat(own), the outlier's own value;
 *   the accept ratio's numerator is (float)(winner + zero_disp), the sum in 64 bits (f2i_sat(own) may be INT_MAX), unless
 *     stm_set_irv_paper_ratio(1) makes it the winning bin's count;  an accepted pixel takes (float)winner. */
void stm_dr_irv(float *disp, unsigned char *outliers, unsigned char **cross, int thresh_s, float thresh_h,
                int num_rows, int num_cols, int num_disp, int zero_disp, int usd, int iterations);
void stm_d_dr_irv(float *d_disp, unsigned char *d_outliers, unsigned char **d_cross, int thresh_s, float thresh_h,
                  int num_rows, int num_cols, int num_disp, int zero_disp, int usd, int iterations);
/* Outlier interpolation (Mei et al. section 3.4, "proper interpolation", the step after region voting; an addition: the reference
 * has none).  disp is refined in place, outliers (dr_dcc's classes, after dr_irv) and img (the same view's image) are read only.
 * A pixel is reliable iff outliers[p] == 0.  For every other pixel p, 16 directions (dx, dy), y growing downwards, in this order:
 *   (1,0) (2,1) (1,1) (1,2) (0,1) (-1,2) (-1,1) (-2,1) (-1,0) (-2,-1) (-1,-1) (-1,-2) (0,-1) (1,-2) (1,-1) (2,-1)
 * Along a direction p + k (dx, dy), k = 1, 2, ... is visited until it leaves the image; the first reliable pixel met is the
 * direction's candidate (the knight's-move directions skip pixels).  outliers[p] == 2 (occlusion): the candidate with the largest
 * stored value (the farthest surface), folded in the order above -- a candidate v replaces the best so far when there is none yet
 * or v > best, so with NaN in the map the result is NaN iff the first direction that has a candidate carries NaN.  Any other
 * non-zero class (mismatch): the candidate whose pixel is closest in colour to p, |dB| + |dG| + |dR| over the first three channels;
 * a candidate replaces the best so far when there is none yet or its distance is strictly smaller (ties: the earlier direction).
 * No candidate in any direction: p keeps its value.  Reliable pixels are never written and the outlier map is not modified; the
 * values written are copies of values in the map.  Parity is against a numpy statement of these lines (parity unpinned). */
void stm_dr_interp(float *disp, unsigned char *outliers, unsigned char *img, int num_rows, int num_cols, int elem_sz);
void stm_d_dr_interp(float *d_disp, unsigned char *d_outliers, unsigned char *d_img, int num_rows, int num_cols, int elem_sz);
/* d_filter_bilateral.h:17-20 / :13-15  (d_filter_bilateral.cu:517-630) */
/*   colour-table index ci = min(f2i_sat(fabsf(va - vs)), num_disp - 1): a NaN difference takes entry 0, an infinite one or one of
 *   2^31 and more entry num_disp - 1.  w = gs * ck[ci]; norm += w; t = vs * w; res += t: one f32 operation each, taps row-major. */
void stm_filter_bilateral_1(float *img, int radius, float sigma_color, float sigma_spatial,
                            int num_rows, int num_cols, int num_disp);
void stm_d_filter_bilateral_1(float *d_img, int radius, float sigma_color, float sigma_spatial,
                              int num_rows, int num_cols, int num_disp);
/* d_filter_gaussian.h:20-26  (d_filter_gaussian.cu:134-234): grow-only gaussian, out = max(in, blur) */
void stm_filter_gaussian_1(float *img, int radius, float sigma_spatial, int num_rows, int num_cols);
void stm_d_filter_gaussian_1(float *d_img, int radius, float sigma_spatial, int num_rows, int num_cols);
/* d_filter.h:22-28  (d_filter.cu:105-167 and following) */
void stm_filter_bleed_1(unsigned char *img, int radius, int num_rows, int num_cols);
void stm_d_filter_bleed_1(unsigned char *d_img, int radius, int num_rows, int num_cols);
/* d_filter.h:11-16  (d_filter.cu:7-103): 3x3 "median" on int-truncated values; unused by the reference's
 * drivers (image_io.cpp:239-240 are commented out) but part of its stage API */
/*   the selection sort compares f2i_sat of the nine samples and stores the converted values back with every swap */
void stm_filter_median(float *img, int num_rows, int num_cols);
void stm_d_filter_median(float *d_img, int num_rows, int num_cols);

/* --------------------------------------------------------------- DIBR (a18-a23) */
/* d_dibr_occl.h:27-33  (d_dibr_occl.cu:130-218) */
/*   occl_r[clamp(x + f2i_sat(disp_l[x] * 1.0f), 0, W - 1)] = 1;  occl_l[clamp(x + f2i_sat(disp_r[x] * -1.0f), 0, W - 1)] = 1;
 *   both sums without overflow */
void stm_dibr_occl(unsigned char *occl_l, unsigned char *occl_r, float *disp_l, float *disp_r,
                   int num_rows, int num_cols);
void stm_d_dibr_occl(unsigned char *d_occl_l, unsigned char *d_occl_r, float *d_disp_l, float *d_disp_r,
                     int num_rows, int num_cols);
/* d_dibr_occl.h:14-20  (d_dibr_occl.cu:17-112) */
void stm_dibr_occl_to_mask(float *mask_l, float *mask_r, unsigned char *occl_l, unsigned char *occl_r,
                           int num_rows, int num_cols);
void stm_d_dibr_occl_to_mask(float *d_mask_l, float *d_mask_r, unsigned char *d_occl_l, unsigned char *d_occl_r,
                             int num_rows, int num_cols);
/* d_dibr_bwarp.h:22-34  (d_dibr_bwarp.cu:24-180).  Host flavour blurs the mask with gaussian(7,10)
 * (:151), device flavour with gaussian(10,15) (:63).  Neither modifies the caller's masks. */
void stm_dibr_dbm(unsigned char *img_out, unsigned char *img_in_l, unsigned char *img_in_r,
                  float *disp_l, float *disp_r, unsigned char *occl_l, unsigned char *occl_r,
                  float *mask_l, float *mask_r, float shift, int num_rows, int num_cols, int elem_sz);
void stm_d_dibr_dbm(unsigned char *d_img_out, unsigned char *d_img_in_l, unsigned char *d_img_in_r,
                    float *d_disp_l, float *d_disp_r, unsigned char *d_occl_l, unsigned char *d_occl_r,
                    float *d_mask_l, float *d_mask_r, float shift, int num_rows, int num_cols, int elem_sz);
/* Linear sampling (an addition: the reference has none).  dibr_dbm with both backward warps fetched at the fractional warp
 * coordinate instead of the truncated one: the reference's own alu_bilinear_interp (d_alu.cu:45-71) given the untruncated
 * clamped position (d_dibr_bwarp.cu:17 assigns it to an int first, which makes the fetch a nearest one and shifts every view
 * by up to a pixel, SURVEY A-Q20).  One warp of image `in` through map `disp`, mask `mask` and factor s, at pixel (x, y),
 * channel c; f32 throughout, one operation per line, C fmaxf / fminf (a NaN position becomes 0):
 *   sd  = disp[p] * s
 *   fx  = (float)x + sd
 *   fx  = fminf(fmaxf(fx, 0), (float)(W - 1))
 *   x0  = (int)floorf(fx);  x1 = min(x0 + 1, W - 1)
 *   wx  = fx - (float)x0
 *   a   = (float)in[y][x0][c] * (1 - wx)
 *   b   = (float)in[y][x1][c] * wx
 *   top = a + b
 *   smp = (u8)top                       (the vertical weight is 0: the row below is not read)
 *   out = (u8)((float)smp * mask[p])
 * Everything else is dibr_dbm's: s = -shift for the left image through disp_r / mask_r, s = (float)(1.0 - (double)shift) for the
 * right image through disp_l / mask_l, the blend G(1 - mask_r) (host flavour gaussian(7,10), device flavour gaussian(10,15)),
 * the merge with its u8 wrap, the bytes past a pixel's third.  Where disp * s is a whole number the result is dibr_dbm's.
 * Parity is against a numpy statement of these lines (parity unpinned). */
void stm_dibr_dbm_lin(unsigned char *img_out, unsigned char *img_in_l, unsigned char *img_in_r,
                      float *disp_l, float *disp_r, unsigned char *occl_l, unsigned char *occl_r,
                      float *mask_l, float *mask_r, float shift, int num_rows, int num_cols, int elem_sz);
void stm_d_dibr_dbm_lin(unsigned char *d_img_out, unsigned char *d_img_in_l, unsigned char *d_img_in_r,
                        float *d_disp_l, float *d_disp_r, unsigned char *d_occl_l, unsigned char *d_occl_r,
                        float *d_mask_l, float *d_mask_r, float shift, int num_rows, int num_cols, int elem_sz);
/* d_dibr_fwarp.h:12-20  (d_dibr_fwarp.cu:27-193): racy in the reference; deterministic here
 * (largest source x wins), parity unpinned */
/*   source x lands on column clamp(x + f2i_sat(disp_l[x] * shift), 0, W - 1), the sum without overflow; the f32 product may be
 *   +-inf (saturates) or NaN (inf * 0: column x) */
void stm_dibr_dfm(unsigned char *img_out, unsigned char *img_in_l, unsigned char *img_in_r,
                  float *disp_l, float *disp_r, float shift, int num_rows, int num_cols, int elem_sz);
void stm_d_dibr_dfm(unsigned char *d_img_out, unsigned char *d_img_in_l, unsigned char *d_img_in_r,
                    float *d_disp_l, float *d_disp_r, float shift, int num_rows, int num_cols, int elem_sz);

/* ---------------------------------------------------------------- mux (a24, a25) */
/* d_mux_multiview.h:35-41  (d_mux_multiview.cu:126-220) */
void stm_mux_multiview(unsigned char **views, unsigned char *out_data, int num_views, float angle,
                       int in_rows, int in_cols, int out_rows, int out_cols, int elem_sz);
void stm_d_mux_multiview(unsigned char **d_views, unsigned char *d_out_data, int num_views, float angle,
                         int in_rows, int in_cols, int out_rows, int out_cols, int elem_sz);
/* Calibrated lenticular interlacing (an addition: the reference's interlacer, mux_multiview_kernel_2 d_mux_multiview.cu:60-73, fixes
 * the lens pitch at exactly num_views sub-pixels, has no phase offset and rounds the slant's row period to an integer -- it fits
 * one panel).  A lenticular panel is calibrated by three numbers:
 *   pitch   (double) sub-pixels per lens
 *   slope   (double) the lens shift in sub-pixels per output row
 *   centre  (double) the phase offset in lenses
 * and `mode` selects what a sub-pixel shows.  Take output pixel (tx, ty) and byte c of the pixel.  Its sub-pixel index is
 * k = 2 - c: R is the first sub-pixel, as in the reference, where R takes r_view, G r_view + 1 and B r_view + 2.  Everything is
 * double, one operation per line, with no contraction:
 *   s  = 3*tx + k                      (int)
 *   t1 = (double)ty * slope
 *   t2 = (double)s + t1
 *   t3 = t2 / pitch                    (correctly rounded)
 *   t4 = t3 + centre
 *   a  = t4 - floor(t4);  if (a >= 1.0) a = 0.0          a in [0,1): the sub-pixel's lens phase
 * (a t4 that is not finite -- a slope or centre at the end of the double range -- gives a = 0 as well.)
 * (xs, ys) and the 4-neighbour sampler are the reference's own (fast_bilinear_interp, d_mux_multiview.cu:10-36), as in
 * stm_mux_multiview; below bilinear_u8(view, c, xs, ys) is that sampler on byte c.  N = num_views.
 * mode 1, nearest view:
 *   g = a * (double)N
 *   v = min((int)g, N - 1)
 *   out = bilinear_u8(views[v], c, xs, ys)
 * mode 2, blended:
 *   g  = a * (double)N
 *   g  = g - 0.5
 *   g  = min(max(g, 0.0), (double)(N - 1))
 *   v0 = min((int)g, N - 2)
 *   w  = (float)(g - (double)v0)
 *   A  = bilinear_u8(views[v0], c, xs, ys);  B = bilinear_u8(views[v0 + 1], c, xs, ys)
 *   p  = (float)A * (1.0f - w)
 *   q  = (float)B * w
 *   out = (u8)(p + q)
 * The half-bin at either lens edge shows the end view unblended: the two end views are never mixed.
 * mode 3, continuous (the frame calls only: it needs the renderer, there are no views):
 *   g as in mode 2 after the clamp
 *   u = g / (double)(N - 1)
 *   shift = (float)(1.0 - u)
 * and a sample at (x, y, c) is the renderer's general form at this shift: shift_l = -shift, shift_r = (float)(1.0 - (double)shift),
 * both backward warps (truncating, or linear as frame bit 0x800 says), the masks, the blend, the u8 wrap (stm_dibr_dbm /
 * stm_dibr_dbm_lin with the frame's gaussian(10, 15) blend), without the shortcut that makes views 0 and N - 1 the two images.
 * The four neighbours are combined as fast_bilinear_interp does; a neighbour of weight exactly 0 need not be evaluated.  At a bin
 * centre (g a whole number) the shift is the discrete view's own, so mode 3 is the limit of mode 2.
 * Argument rules: mode in 0 .. 3 (0 = off: the other arguments are ignored), pitch finite and >= 1, slope and centre finite,
 * num_views >= 2.  Anything else fails through stm_last_error before anything is launched or written.
 *
 * The per-stage calls accept modes 1 and 2 (0 and 3 are errors).  Pixel format as stm_mux_multiview: the first three bytes of a
 * pixel; the host flavour zeroes the padding, the device flavour leaves it alone.  Parity is against a numpy statement of these
 * lines (parity unpinned). */
void stm_mux_multiview_lens(unsigned char **views, unsigned char *out_data, int num_views, int mode, double pitch, double slope,
                            double centre, int in_rows, int in_cols, int out_rows, int out_cols, int elem_sz);
void stm_d_mux_multiview_lens(unsigned char **d_views, unsigned char *d_out_data, int num_views, int mode, double pitch, double slope,
                              double centre, int in_rows, int in_cols, int out_rows, int out_cols, int elem_sz);

/* The views tiled into one frame, a quilt (an addition; the counterpart of stm_mux_multiview_lens for a display that does its own
 * interlacing).  views = table of num_views images in_rows x in_cols x elem_sz, views[0] = the right image ... views[num_views-1]
 * = the left image, as the interlacer takes them; V(v, x, y, c) is byte c of pixel (x, y) of views[v].
 *   tiles_x, tiles_y >= 1 with tiles_x * tiles_y == num_views
 *   order    bit 0: tile rows run bottom-up (the Looking Glass convention); bit 1: the view order is reversed, so tile 0 holds the
 *            leftmost camera (view num_views-1)
 *   filter   0 = the reference's four-neighbour sampler (fast_bilinear_interp), 1 = the area average
 * Geometry, with N = num_views, the output Hout x Wout and the views Hin x Win, integer division:
 *   tw = Wout / tiles_x;  th = Hout / tiles_y                      the size of a tile (both must be >= 1)
 *   k  = (order & 2) ? N - 1 - v : v                               the tile view v goes to
 *   i  = k % tiles_x;  j = k / tiles_x
 *   left = i * tw                                                  the tile's left column
 *   top  = (order & 1) ? Hout - (j + 1) * th : j * th              the tile's top row
 * The Wout - tiles_x * tw remainder columns at the right and the Hout - tiles_y * th remainder rows -- at the bottom when top-down, at
 * the top when bottom-up -- belong to no tile: bytes 0 .. 2 of such a pixel are written 0.  All three bytes of a tile pixel come
 * from the same view.  For tile pixel (u, w), 0 <= u < tw, 0 <= w < th, at output pixel (left + u, top + w):
 * Filter 0 (f32, one operation per line, C fminf / fmaxf -- mux_multiview_kernel_2's lines with the tile's size for the frame's):
 *   xs = ((float)u / (float)tw) * (float)Win;  xs = fminf(fmaxf(xs, 0), (float)(Win - 1))
 *   ys = ((float)w / (float)th) * (float)Hin;  ys = fminf(fmaxf(ys, 0), (float)(Hin - 1))
 *   out[c] = fast_bilinear_interp of V(v, ., ., c) at (xs, ys)     (d_mux_multiview.cu:10-36)
 * Filter 1 (unsigned integers wide enough for 255 * Win * Hin, `/` the integer division; any summation order gives the same bits).
 * In units of 1/tw of a view pixel tile column u covers [u Win, (u+1) Win) and view column x covers [x tw, (x+1) tw):
 *   wx(x) = max(0, min((u+1) Win, (x+1) tw) - max(u Win, x tw))    non-zero for x = u Win / tw .. ((u+1) Win - 1) / tw; sum = Win
 *   wy(y) = max(0, min((w+1) Hin, (y+1) th) - max(w Hin, y th))    non-zero for y = w Hin / th .. ((w+1) Hin - 1) / th; sum = Hin
 *   out[c] = (sum_y sum_x wy(y) wx(x) V(v, x, y, c) + (Win Hin) / 2) / (Win Hin)
 * the exact mean of the view over the tile pixel's footprint, rounded half up.  With tw >= Win the footprint is at most two view
 * columns (a tile pixel inside one view pixel copies it); the same lines define that case.
 * Pixel format: as stm_mux_multiview -- the host flavour returns bytes 3 .. elem_sz-1 as 0, the device flavour leaves them alone.
 * Errors, through stm_last_error with nothing launched: a dimension < 1, elem_sz < 3, num_views < 2, order or filter out of range,
 * tiles_x * tiles_y != num_views, a tile of width or height 0, tw * in_cols or th * in_rows >= 2^31. */
void stm_quilt_multiview(unsigned char **views, unsigned char *out_data, int num_views, int tiles_x, int tiles_y, int order, int filter,
                         int in_rows, int in_cols, int out_rows, int out_cols, int elem_sz);
void stm_d_quilt_multiview(unsigned char **d_views, unsigned char *d_out_data, int num_views, int tiles_x, int tiles_y, int order, int filter,
                           int in_rows, int in_cols, int out_rows, int out_cols, int elem_sz);
/* An overlay composited into a finished frame at a chosen depth (an addition: the reference has nowhere to put subtitles, a logo or
 * a player's OSD; painted on the finished frame they are pinned to the screen plane, and on a quilt they would have to be drawn once
 * per tile with offsets derived from this library's internals).  The overlay is a small image in VIEW PIXEL SPACE:
 *   overlay    ov_rows x ov_cols pixels of 4 bytes B, G, R, A with PREMULTIPLIED alpha (colour <= alpha expected), dense, read only;
 *              O[r][q] is its pixel at row r, column q
 *   x0, y0     the view pixel its top-left corner sits at (either may be negative or beyond the view: the overlay is clipped)
 *   disparity  one end-to-end disparity in the maps' sign convention (x_right - x_left): > 0 behind the screen, < 0 in front, 0 on it
 * View pixel space, Hv x Wv:
 *   layout 0          the output frame, out_rows x out_cols
 *   layout 1 (quilt)  one tile, th x tw (stm_quilt_multiview's geometry); the overlay is composited into every tile, clipped to that
 *                     tile; the remainder pixels that belong to no tile are never touched
 * The overlay is drawn at the output's own resolution (text stays as sharp as the panel); it is not resampled vertically.
 * Take view pixel (x, y) and byte c (0 .. 2) of that pixel; in a quilt (x, y) = (u, w) inside the tile of view v, at output pixel
 * (left + u, top + w); in layout 0 the output pixel is (x, y) itself.  N = num_views.
 * 1. The sub-pixel's shift s, the camera position it shows (1 = the right image, 0 = the left image):
 *   layout 0, lens mode 0   v = the view the frame's interlacer shows there: mux_multiview_kernel_2's b_view, g_view, r_view for c = 0,
 *                           1, 2 (d_mux_multiview.cu:60-73, the form that multiplies by 1 / y_interval, which the frame calls use), from
 *                           `angle`;  s = (float)(1.0 - (double)(float)v / ((double)(float)N - 1.0))            (d_io.cu:189)
 *   lens mode 1             v by stm_mux_multiview_lens's mode 1 lines at output pixel (x, y), byte c; then the same s
 *   lens modes 2 and 3      mode 3's shift at output pixel (x, y), byte c: g after the clamp, u = g / (double)(N - 1), s = (float)(1.0 - u).
 *                           The overlay is drawn at the sub-pixel's own continuous position, in mode 2 as well
 *   layout 1                v = the tile's view; then the same s as for a discrete view
 *   The depth budget (stm_set_depth) does not enter: `disparity` is end-to-end.  A caller who wants it relative to the scene reads
 *   stm_stream_depth.
 * 2. The position.  double, one operation per line, no contraction:
 *   t  = (double)s - 0.5
 *   o  = (double)disparity * t
 *   p  = (double)(x - x0) - o                  (x - x0 in 64-bit integers)
 *   p  = p * 256.0
 *   F  = (long long)floor(p)
 *   q  = F >> 8 (arithmetic);  fr = F & 255
 *   r  = y - y0;  r outside [0, ov_rows): the sub-pixel is unchanged
 *   So overlay pixel q' appears at x0 + q' + (s - 0.5) * disparity.
 * 3. The sample.  P0 = O[r][q], P1 = O[r][q + 1]; a column outside [0, ov_cols) reads as (0, 0, 0, 0).  For byte j of the overlay pixel
 *   I_j = (256 - fr) * P0_j + fr * P1_j                                                        (0 .. 65280)
 * 4. The blend.  Unsigned 32-bit integers, `/` the integer division; the numerator stays below 2^26:
 *   out = min(255, (255 * I_c + (65280 - I_3) * dst + 32640) / 65280)
 *   I_c = I_3 = 0 leaves dst exactly; full alpha (I_3 = 65280) gives I_c / 256 exactly; the result stays in 0 .. 255 for every
 *   premultiplied pixel, so the min only guards an overlay that is not (colour > alpha).
 * Bytes 3 .. elem_sz - 1 of an output pixel are never written.  Only sub-pixels inside the bounding box can change, and only they are
 * visited: view rows [max(0, y0), min(Hv, y0 + ov_rows)), view columns [x0 - m, x0 + ov_cols + m) within [0, Wv), m =
 * ceil(|disparity| / 2) + 1; an empty box launches nothing.  The device flavour composites in place on a finished frame of the stated
 * geometry and writes only bytes 0 .. 2 of the pixels inside the box; the frame and the overlay may not overlap; the frame may have
 * any byte alignment.  The host flavour uploads the frame and the overlay, composites, and downloads the frame (every byte of it
 * comes back as it went in, except what the compositor wrote).
 * Geometry arguments: num_views, angle (lens mode 0 with layout 0 only), the lens (lens_mode 0 .. 3 with stm_set_lens's rules; mode 3
 * is allowed here: it needs no views), the layout (0, or 1 with tiles_x, tiles_y, order and stm_quilt_multiview's rules; a lens mode
 * != 0 with layout 1 is an error), out_rows, out_cols, elem_sz.
 * Errors, through stm_last_error with nothing launched or written: a null or not 4-byte aligned overlay; ov_rows or ov_cols outside
 * 1 .. 65535; |x0| or |y0| > 65536; a disparity that is not finite or of magnitude > 4096; out_rows or out_cols < 1, elem_sz < 3,
 * num_views < 2; the lens rules; the layout rules (tiles_x * tiles_y != num_views, a tile of width or height 0, more than 65535 tiles);
 * in lens mode 0 with layout 0 an angle whose tangent is 0 or too steep, as stm_mux_multiview.
 * Out of scope: NV12 output (compositing on a chroma-subsampled surface needs a definition of its own: the frame calls and the frame
 * stream refuse the combination), animated or several simultaneous overlays (a caller flattens them into one), vertical resampling,
 * straight alpha (convert first).  Parity is against a numpy statement of these lines (parity unpinned). */
void stm_mux_overlay(unsigned char *frame, const unsigned char *overlay, int ov_rows, int ov_cols, int x0, int y0, float disparity,
                     int num_views, float angle, int lens_mode, double pitch, double slope, double centre, int layout, int tiles_x,
                     int tiles_y, int order, int out_rows, int out_cols, int elem_sz);
void stm_d_mux_overlay(unsigned char *d_frame, const unsigned char *d_overlay, int ov_rows, int ov_cols, int x0, int y0, float disparity,
                       int num_views, float angle, int lens_mode, double pitch, double slope, double centre, int layout, int tiles_x,
                       int tiles_y, int order, int out_rows, int out_cols, int elem_sz);
/* d_demux_common.h:10-13  demux_sbs kernel (d_demux_common.cu:8-33) as a host-callable stage */
void stm_d_demux_sbs(unsigned char *d_img_l, unsigned char *d_img_r, unsigned char *d_img_sbs,
                     int num_rows, int num_cols_sbs, int num_cols_out, int elem_sz);
/* NV12 input (an addition: the reference takes one side-by-side BGR frame per call, which no video decoder delivers).  Colour
 * conversion + split as a stage: the counterpart of stm_d_demux_sbs for a side-by-side NV12 frame of num_rows rows and
 * num_cols_sbs columns, the left view in columns [0, W) and the right view in [W, 2 W), W = num_cols_out.
 *   y    u8, num_rows rows of pitch_y bytes.
 *   uv   u8, num_rows / 2 rows of pitch_uv bytes; bytes 2k and 2k + 1 of a row are U and V of the 2 x 2 luma block at columns 2k, 2k + 1.
 * num_rows and W must be even (each half starts on a chroma sample), num_cols_sbs >= 2 W, pitch_y >= num_cols_sbs,
 * pitch_uv >= 2 * ((num_cols_sbs + 1) / 2).  The base pointers may have any byte alignment.  Both planes are read only.
 * Chroma is replicated: pixel (x, y) of the frame uses U = uv[y >> 1][2 (x >> 1)], V = uv[y >> 1][2 (x >> 1) + 1].
 * `matrix` selects a row of coefficients: 0 = BT.601 limited range, 1 = BT.709 limited, 2 = BT.601 full, 3 = BT.709 full.
 * All arithmetic is 32-bit signed integer, >> an arithmetic shift (floor):
 *   C = Y - yo;  D = U - 128;  E = V - 128
 *   B = clip255((ky*C + bu*D        + 32768) >> 16)
 *   G = clip255((ky*C - gu*D - gv*E + 32768) >> 16)
 *   R = clip255((ky*C + rv*E        + 32768) >> 16)
 * With (Kr, Kb) = (0.299, 0.114) for 601 and (0.2126, 0.0722) for 709, Kg = 1 - Kr - Kb, and (ky, s, yo) = (255/219, 255/224, 16)
 * for limited and (1, 1, 0) for full range: rv = 2(1-Kr)s, bu = 2(1-Kb)s, gu = 2Kb(1-Kb)s/Kg, gv = 2Kr(1-Kr)s/Kg, each times
 * 65536 in double and rounded to nearest (none is a tie):
 *   matrix   ky      rv      gu     gv      bu
 *     0     76309  104597  25675  53279  132201
 *     1     76309  117489  13975  34925  138438
 *     2     65536   91881  22553  46802  116130
 *     3     65536  103206  12276  30679  121609
 * No intermediate exceeds 2^26.  E.g. matrix 0: (Y, U, V) = (16,128,128) -> (B, G, R) = (0,0,0); (235,128,128) -> (255,255,255);
 * (81,90,240) -> (0,0,254); (0,0,0) -> (0,136,0); (255,0,255) -> (20,225,255).
 * img_l / img_r are num_rows x W x elem_sz with B, G, R in a pixel's first three bytes; the bytes past the third come back 0
 * from the host flavour and are left as they were by the device flavour.  Errors (stm_last_error), all reported before anything is
 * launched or written: an odd num_rows or num_cols_out, num_cols_sbs < 2 W, a pitch below the rules, matrix outside 0 .. 3.
 * Parity is against a numpy statement of these lines (parity unpinned). */
void stm_demux_nv12(unsigned char *img_l, unsigned char *img_r, unsigned char *y, int pitch_y, unsigned char *uv, int pitch_uv,
                    int num_rows, int num_cols_sbs, int num_cols_out, int elem_sz, int matrix);
void stm_d_demux_nv12(unsigned char *d_img_l, unsigned char *d_img_r, unsigned char *d_y, int pitch_y, unsigned char *d_uv, int pitch_uv,
                      int num_rows, int num_cols_sbs, int num_cols_out, int elem_sz, int matrix);
/* NV12 output (an addition; the counterpart of stm_demux_nv12 for what an encoder takes).  Colour conversion as a stage: the NV12
 * picture of a BGR image img (num_rows x num_cols x elem_sz, B, G, R in a pixel's first three bytes; H = num_rows and W = num_cols
 * even and >= 2).  The image is read through the bytes as stored: for a quilt, the rounded u8 output of stm_quilt_multiview's rules,
 * pad pixels 0 included.  The conversion does not read the filter's unrounded accumulators.
 *   y    u8, H rows of pitch_y bytes.
 *   uv   u8, H / 2 rows of pitch_uv bytes; bytes 2k and 2k + 1 of row j are U and V of the 2 x 2 block at rows 2j, 2j + 1 and columns
 *        2k, 2k + 1.
 * All arithmetic is 32-bit signed integer.  >> is an arithmetic shift.
 *   Y[y][x]       = clip255((yr*R + yg*G + yb*B + (yo << 16) + 32768) >> 16)
 *   SB, SG, SR    = the sums of B, G, R over the block rows 2j, 2j+1 x columns 2k, 2k+1      (0 .. 1020)
 *   UV[j][2k]     = clip255((h*SB - ug*SG - ur*SR + (128 << 18) + (1 << 17)) >> 18)         (U)
 *   UV[j][2k + 1] = clip255((h*SR - vg*SG - vb*SB + (128 << 18) + (1 << 17)) >> 18)         (V)
 * So chroma is the exact mean of the four pixels' chroma, rounded once (centre siting).  This is the counterpart of the input side's
 * replicated chroma.
 * Coefficients use stm_demux_nv12's (Kr, Kb) and range per `matrix` 0 .. 3.  (sy, sc, yo) is (219/255, 224/255, 16) for limited range
 * and (1, 1, 0) for full range.  Each rounded coefficient is computed in double and rounded to nearest (none is a tie):
 *   ys = round(65536 sy), yr = round(65536 Kr sy), yb = round(65536 Kb sy), yg = ys - yr - yb
 *   h = round(32768 sc), ur = round(65536 Kr sc / (2 (1 - Kb))), ug = h - ur
 *   vb = round(65536 Kb sc / (2 (1 - Kr))), vg = h - vb
 * The three derived coefficients make white land exactly on 235 / 255.  They also make every grey give U = V = 128 exactly.
 *   matrix  yo    yr     yg     yb     h      ur     ug     vg     vb
 *     0     16  16829  33039   6416  28784   9714  19070  24103   4681
 *     1     16  11966  40254   4064  28784   6596  22188  26145   2639
 *     2      0  19595  38470   7471  32768  11058  21710  27439   5329
 *     3      0  13933  46871   4732  32768   7509  25259  29763   3005
 * Known answers for a uniform 2 x 2 block, (B, G, R) -> (Y, U, V).  Matrix 0: (0,0,0) -> (16,128,128); (255,255,255) -> (235,128,128);
 * (0,0,255) -> (81,90,240); (255,0,0) -> (41,240,110); (0,255,0) -> (145,54,34).  Matrix 2: (255,0,0) -> (29,255,107), where U is
 * clipped from 256.  Matrix 3: (0,255,0) -> (182,30,12).
 * No intermediate exceeds 2^26.  Y never needs its clip.  Chroma needs only the clip at 256.
 * Rules: num_rows and num_cols even and >= 2, pitch_y >= num_cols, pitch_uv >= num_cols, matrix in 0 .. 3, elem_sz >= 3.  The base
 * pointers may have any byte alignment.  img is read only.  The device flavour leaves every byte of the two planes that is not a
 * sample as it was; the host flavour returns the bytes between a row's samples and the next row as 0.  Errors (stm_last_error), all
 * reported before anything is launched or written.  Parity is against a numpy statement of these lines (parity unpinned).
 * Out of scope: left-co-sited chroma, P010 / 10-bit, planar I420. */
void stm_mux_nv12(unsigned char *y, int pitch_y, unsigned char *uv, int pitch_uv, unsigned char *img, int num_rows, int num_cols,
                  int elem_sz, int matrix);
void stm_d_mux_nv12(unsigned char *d_y, int pitch_y, unsigned char *d_uv, int pitch_uv, unsigned char *d_img, int num_rows, int num_cols,
                    int elem_sz, int matrix);
/* Packed stereo frames (an addition: the reference takes two full-resolution eyes side by side, left first, a layout almost no stereo
 * video is stored in).  The unpacking as a stage: the counterpart of stm_d_demux_sbs for a frame in one of the common packings.
 *   packing  0 = side by side, full;  1 = side by side, each eye squeezed to half the columns;
 *            2 = top and bottom, full;  3 = top and bottom, each eye squeezed to half the rows.
 *   swap     0 or 1: the right eye comes first.
 *   filter   0 = linear, 1 = Catmull-Rom: how a squeezed eye is expanded (packings 1 and 3 only; with 0 and 2 it must be 0).
 *   gap      >= 0 (at most 2^24): pixels between the two eyes along the packing axis -- columns for packings 0 and 1, rows for 2 and 3
 *            (HDMI / Blu-ray frame packing is packing 2 with the blank band as the gap).
 * H = num_rows and W = num_cols_out are the size of an eye AFTER unpacking.  The packed eye is Hp x Wp, the frame has rows_f rows of
 * num_cols_sbs pixels:
 *   packing   Hp x Wp      rows_f        required row length
 *      0      H x W        H             num_cols_sbs >= 2 W + gap
 *      1      H x W/2      H             num_cols_sbs >= 2 Wp + gap
 *      2      H x W        2 H + gap     num_cols_sbs >= W
 *      3      H/2 x W      2 Hp + gap    num_cols_sbs >= W
 * Eye e (0 = left, 1 = right) is the q-th in the frame, q = e ^ swap; its origin (row, column) is
 *   (0, q (Wp + gap))   for packings 0 and 1
 *   (q (Hp + gap), 0)   for packings 2 and 3.
 * Packings 0 and 2 copy.  Packings 1 and 3 expand by two along one axis (x for 1, y for 3).  P = the packed eye along that axis, n
 * samples; every index is clamped to [0, n - 1] of the eye's own region, never into the gap or the other eye.  Per byte B, G, R, for
 * output index x, in 32-bit signed integers, >> an arithmetic shift:
 *   k = x >> 1;  s = +1 if x is odd, else -1
 *   out = clip255((w0 P[k - s] + w1 P[k] + w2 P[k + s] + w3 P[k + 2 s] + 64) >> 7)
 *   (w0, w1, w2, w3) = (0, 96, 32, 0)      filter 0: exactly (3 P[k] + P[k + s] + 2) >> 2
 *                      (-9, 111, 29, -3)   filter 1
 * These are the half-pixel-centred 2 x up-sampling positions k -+ 1/4 of the linear and the Catmull-Rom kernels (the latter's weights
 * at 1/4 are whole multiples of 1/128); both sets sum to 128, so a constant eye is reproduced exactly; a tap of weight 0 need not be read.
 * Pixel format as stm_demux_nv12: img_l / img_r are H x W x elem_sz with B, G, R in a pixel's first three bytes, of the frame only
 * the first three bytes of a pixel are read; the bytes past the third come back 0 from the host flavour and are left as they were
 * by the device flavour.  The frame is read only and may have any byte alignment.
 * stm_demux_nv12_packed takes stm_demux_nv12's planes and matrix: the result is by definition the unpacking above applied to the BGR
 * picture that stm_demux_nv12's conversion gives on the PACKED frame -- chroma replicated at packed resolution, in frame coordinates:
 * frame pixel (row, col) uses uv[row >> 1][2 (col >> 1)], [.. + 1].  y has rows_f rows, uv rows_f / 2.  Every eye origin and Wp, Hp
 * must be even: W and H even, W % 4 == 0 for packing 1, H % 4 == 0 for packing 3, gap even; pitch_y >= num_cols_sbs, pitch_uv >=
 * 2 * ((num_cols_sbs + 1) / 2).
 * Errors (stm_last_error), all reported before anything is launched or written: a setting outside its range; filter != 0 with
 * packing 0 or 2 (an error, not ignored); an odd W with packing 1, an odd H with packing 3; a row length or a pitch below the rule;
 * the NV12 evenness rules; matrix outside 0 .. 3.  Parity is against a numpy statement of these lines (parity unpinned). */
void stm_demux_packed(unsigned char *img_l, unsigned char *img_r, unsigned char *img, int num_rows, int num_cols_sbs, int num_cols_out,
                      int elem_sz, int packing, int swap, int filter, int gap);
void stm_d_demux_packed(unsigned char *d_img_l, unsigned char *d_img_r, unsigned char *d_img, int num_rows, int num_cols_sbs,
                        int num_cols_out, int elem_sz, int packing, int swap, int filter, int gap);
void stm_demux_nv12_packed(unsigned char *img_l, unsigned char *img_r, unsigned char *y, int pitch_y, unsigned char *uv, int pitch_uv,
                           int num_rows, int num_cols_sbs, int num_cols_out, int elem_sz, int matrix, int packing, int swap, int filter,
                           int gap);
void stm_d_demux_nv12_packed(unsigned char *d_img_l, unsigned char *d_img_r, unsigned char *d_y, int pitch_y, unsigned char *d_uv,
                             int pitch_uv, int num_rows, int num_cols_sbs, int num_cols_out, int elem_sz, int matrix, int packing, int swap,
                             int filter, int gap);

/* ------------------------------------------------------------ whole frame (a26) */
/* d_io.h:32-40  adcensus_stm (d_io.cu:7-238).  `angle` is float here (the reference's int truncates
 * the caller's float, SURVEY A-Q24). */
void stm_adcensus_stm(unsigned char *img_sbs, float *disp_l, float *disp_r, unsigned char *interlaced,
                      int num_rows, int num_cols_sbs, int num_cols,
                      int num_rows_out, int num_cols_out, int elem_sz,
                      int num_views, float angle, int num_disp, int zero_disp,
                      float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd,
                      int thresh_s, float thresh_h);
/* Device-resident frame: same pipeline, all four buffers already in HBM, nothing synchronised.
 * stages: 1 = cost init + aggregation + WTA only (BASELINE config 2);
 *         2 = + DCC / IRV x5 / bilateral          (config 3);
 *         3 = + DIBR views + interlacing           (config 4, the full adcensus_stm).
 * OR-ing 0x100 inserts the scanline optimisation (HSLO, constants of image_io.cpp:311-313) between aggregation
 * and WTA for both views, as Mei et al. order it; the reference never wires it in (parity unpinned).
 * OR-ing 0x200 adds the sub-pixel enhancement of stm_dc_subpixel on the aggregated costs of each view: with stages 1 on the
 * WTA maps; with stages 2 and 3 after region voting and before the bilateral filter (DCC and IRV still see whole numbers;
 * stage 3 renders from the refined, filtered maps).  Parity: the oracle chain with a numpy statement of the step.  0x200
 * together with 0x100 is an error (stm_last_error), reported before anything is launched.
 * OR-ing 0x400 adds the outlier interpolation of stm_dr_interp to stages 2 and 3: after region voting, before the sub-pixel step
 * and the bilateral filter, each view on its own image and its own post-voting outlier map.  It combines with 0x100 and with
 * 0x200 (order: voting, interpolation, sub-pixel, bilateral).  With stages 1 there are no outlier maps: 1 | 0x400 is an error
 * (stm_last_error), reported before anything is launched.
 * OR-ing 0x800 renders the views of stage 3 with the linear sampling of stm_dibr_dbm_lin instead of the truncating fetch; the
 * disparity maps are the same with and without it.  It combines with 0x100, 0x200 and 0x400.  Stages 1 and 2 render nothing:
 * 1 | 0x800 and 2 | 0x800 are errors (stm_last_error), reported before anything is launched.  stm_adcensus_stm and the two
 * adcensus_stm_2 calls keep the truncating fetch.
 * 0x1000 (guided up-sampling) belongs to the reduced-resolution frame, stm_d_adcensus_stm_2s: here it is an error.
 * 0x2000 (temporal stabilisation) needs the previous frame, which this call has no arguments for: here, and in the two _2s
 * calls, it is an error; stm_d_adcensus_stm_t takes it. */
void stm_d_adcensus_stm(unsigned char *d_img_sbs, float *d_disp_l, float *d_disp_r, unsigned char *d_interlaced,
                        int num_rows, int num_cols_sbs, int num_cols,
                        int num_rows_out, int num_cols_out, int elem_sz,
                        int num_views, float angle, int num_disp, int zero_disp,
                        float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd,
                        int thresh_s, float thresh_h, int stages);
/* The device-resident frame of a frame sequence (an addition): stm_d_adcensus_stm's arguments and rules plus the history of the
 * temporal stabilisation, stage bit 0x2000: d_prev_img_sbs, the previous frame's side-by-side input (same geometry as
 * d_img_sbs), d_prev_disp_l / d_prev_disp_r, the two maps the previous frame put out (its stabilised result), and
 * stm_disp_temporal's three parameters.  With the bit set and all three history pointers non-null, stm_disp_temporal runs on
 * d_disp_l and d_disp_r in place after the bilateral filter and before the renderer, each view on its own half of the two
 * side-by-side buffers (a view's 3 x 3 neighbourhood is clipped to its own half): stages 2 | 0x2000 returns the stabilised maps,
 * 3 | 0x2000 renders from them.  The bit combines with 0x100, 0x200, 0x400 and 0x800.  With the bit set and all three pointers
 * null (the first frame of a sequence) nothing extra is launched: the call is stm_d_adcensus_stm without the bit, bit for bit.
 * Without the bit the history arguments are ignored.  Errors (stm_last_error), all reported before anything is launched: some
 * history pointers null and some not; a low byte of `stages` below 2; num_cols_sbs < 2 * num_cols; a history map that overlaps
 * d_disp_l or d_disp_r; alpha, thresh_color or thresh_disp outside stm_disp_temporal's rules (checked whenever the bit is set).
 * The defaults a frame sequence uses (stm_stream_set_temporal): alpha = 0.5, thresh_color = 24, thresh_disp = 1.5.  Why 24:
 * sensor noise of +-2 per channel and frame gives |delta| <= 4 per channel, so sad <= 12: a static noisy pixel stays inside
 * the gate with a factor of two to spare. */
void stm_d_adcensus_stm_t(unsigned char *d_img_sbs, float *d_disp_l, float *d_disp_r, unsigned char *d_interlaced,
                          int num_rows, int num_cols_sbs, int num_cols,
                          int num_rows_out, int num_cols_out, int elem_sz,
                          int num_views, float angle, int num_disp, int zero_disp,
                          float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd,
                          int thresh_s, float thresh_h, int stages,
                          unsigned char *d_prev_img_sbs, float *d_prev_disp_l, float *d_prev_disp_r,
                          float alpha, int thresh_color, float thresh_disp);
/* The device-resident frame on an NV12 frame (an addition): by definition stm_d_adcensus_stm_t applied to the side-by-side BGR frame
 * that stm_demux_nv12's conversion gives, with every rule of `stages` unchanged; the conversion runs inside the frame's first
 * kernel, no BGR frame is materialised.  Arguments as stm_d_adcensus_stm_t, except:
 *   d_img_sbs      becomes d_y, pitch_y, d_uv, pitch_uv, matrix (stm_demux_nv12's layout and rules; num_cols_sbs >= 2 * num_cols
 *                  is required whatever the stages);
 *   d_prev_img_sbs becomes d_prev_img_l, d_prev_img_r: the previous frame's converted split images (num_rows x num_cols x elem_sz);
 *   d_img_l, d_img_r (last) receive this frame's converted split images, in the device flavour's form (bytes past a pixel's third
 *                  are left alone).  Both null: they stay in the workspace.  With 0x2000 both must be given: this frame's images
 *                  are the next frame's history.
 * With the bit set and all four history pointers null (the first frame) the call is the one without the bit.  Errors
 * (stm_last_error), all reported before anything is launched or written: what stm_demux_nv12 and stm_d_adcensus_stm_t refuse;
 * exactly one of d_img_l / d_img_r null; 0x2000 without them; some history pointers null and some not; a history buffer that
 * overlaps d_img_l, d_img_r, d_disp_l or d_disp_r. */
void stm_d_adcensus_stm_nv12(unsigned char *d_y, int pitch_y, unsigned char *d_uv, int pitch_uv, int matrix,
                             float *d_disp_l, float *d_disp_r, unsigned char *d_interlaced,
                             int num_rows, int num_cols_sbs, int num_cols,
                             int num_rows_out, int num_cols_out, int elem_sz,
                             int num_views, float angle, int num_disp, int zero_disp,
                             float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd,
                             int thresh_s, float thresh_h, int stages,
                             unsigned char *d_prev_img_l, unsigned char *d_prev_img_r, float *d_prev_disp_l, float *d_prev_disp_r,
                             float alpha, int thresh_color, float thresh_disp,
                             unsigned char *d_img_l, unsigned char *d_img_r);

/* Reduced-resolution disparity: d_io.h:42-52 adcensus_stm_2 (d_io.cu:240-508).  The pair is
 * bilinearly reduced to num_rows_disp x num_cols_disp, matched there, and the disparity maps are scaled back up
 * by 1/disp_scale before the views are rendered at full resolution.  `angle` is float (A-Q24). */
void stm_adcensus_stm_2(unsigned char *img_sbs, float *disp_l, float *disp_r, unsigned char *interlaced,
                        int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out,
                        int num_rows_disp, int num_cols_disp, int elem_sz, float disp_scale,
                        int num_views, float angle, int num_disp, int zero_disp,
                        float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd,
                        int thresh_s, float thresh_h);
void stm_d_adcensus_stm_2(unsigned char *d_img_sbs, float *d_disp_l, float *d_disp_r, unsigned char *d_interlaced,
                          int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out,
                          int num_rows_disp, int num_cols_disp, int elem_sz, float disp_scale,
                          int num_views, float angle, int num_disp, int zero_disp,
                          float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd,
                          int thresh_s, float thresh_h);
/* The reduced-resolution frame with a `stages` word (an addition: the reference's call has none).  Arguments as the two calls
 * above plus `stages`, whose low byte must be 3 (this path always renders) and which may carry, with stm_d_adcensus_stm's rules
 * (0x200 | 0x100 is an error):
 *   0x100, 0x200, 0x400  HSLO, sub-pixel enhancement, outlier interpolation of the match on the reduced pair;
 *   0x800                linear sampling of the warps in the full-resolution render;
 *   0x1000               the guided up-sampling of stm_disp_upsample (sigma_color = 15) in place of the bilinear up-scale: the left
 *                        map guided by the full-resolution left image against the reduced left image, the right map alike.
 * Any other value is an error (stm_last_error), reported before anything is launched; the caller's buffers are not touched.
 * stages == 3 is stm_adcensus_stm_2 / stm_d_adcensus_stm_2 bit for bit.  stm_d_adcensus_stm and stm_stream_set_stages reject
 * 0x1000: at full resolution nothing is up-scaled. */
void stm_adcensus_stm_2s(unsigned char *img_sbs, float *disp_l, float *disp_r, unsigned char *interlaced,
                         int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out,
                         int num_rows_disp, int num_cols_disp, int elem_sz, float disp_scale,
                         int num_views, float angle, int num_disp, int zero_disp,
                         float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd,
                         int thresh_s, float thresh_h, int stages);
void stm_d_adcensus_stm_2s(unsigned char *d_img_sbs, float *d_disp_l, float *d_disp_r, unsigned char *d_interlaced,
                           int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out,
                           int num_rows_disp, int num_cols_disp, int elem_sz, float disp_scale,
                           int num_views, float angle, int num_disp, int zero_disp,
                           float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd,
                           int thresh_s, float thresh_h, int stages);
/* The reduced-resolution frame for frame sequences (an addition).  stm_d_adcensus_stm_2t is stm_d_adcensus_stm_2s with the history
 * of the temporal stabilisation: stm_d_adcensus_stm_2s's arguments, then stm_d_adcensus_stm_t's six history arguments.
 *   stages   low byte 3; 0x100, 0x200, 0x400, 0x800, 0x1000 as stm_d_adcensus_stm_2s; 0x2000 = temporal stabilisation with
 *            stm_d_adcensus_stm_t's rules: the three history pointers all null (the first frame: the bit does nothing) or all set, no
 *            history map aliasing d_disp_l / d_disp_r, stm_disp_temporal's parameter rules, num_cols_sbs >= 2 * num_cols with a history.
 * The temporal step runs on the UP-SCALED full-size maps (after tx_disp_scale, or after the guided up-sampler with 0x1000) with the
 * two full-size side-by-side frames, and before the render: the same placement as in the full-resolution frame, on the final maps.
 * So d_prev_disp_l / d_prev_disp_r are the previous call's d_disp_l / d_disp_r (num_rows x num_cols).
 * stm_d_adcensus_stm_2nv12 is the same frame on NV12 planes: stm_d_adcensus_stm_nv12's arguments with num_rows_disp, num_cols_disp
 * after num_cols_out and disp_scale after elem_sz (stm_d_adcensus_stm_2s's places), stm_demux_nv12's geometry rules, and
 * stm_d_adcensus_stm_nv12's rules for the four history pointers and for d_img_l / d_img_r (both or neither; required with 0x2000).
 * The reduced pair is tx_scale_bilinear of the CONVERTED split images.
 * 0x300, any other low byte and any other bit are errors; a packing set on the thread (stm_set_packing) is refused.  Every error is
 * reported (stm_last_error) before anything is launched; the caller's buffers are not touched.  stm_d_adcensus_stm_2s itself keeps
 * rejecting 0x2000.  Without 0x2000 and history, stm_d_adcensus_stm_2t is stm_d_adcensus_stm_2s bit for bit. */
void stm_d_adcensus_stm_2t(unsigned char *d_img_sbs, float *d_disp_l, float *d_disp_r, unsigned char *d_interlaced,
                           int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out,
                           int num_rows_disp, int num_cols_disp, int elem_sz, float disp_scale,
                           int num_views, float angle, int num_disp, int zero_disp,
                           float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd,
                           int thresh_s, float thresh_h, int stages,
                           unsigned char *d_prev_img_sbs, float *d_prev_disp_l, float *d_prev_disp_r,
                           float alpha, int thresh_color, float thresh_disp);
void stm_d_adcensus_stm_2nv12(unsigned char *d_y, int pitch_y, unsigned char *d_uv, int pitch_uv, int matrix,
                              float *d_disp_l, float *d_disp_r, unsigned char *d_interlaced,
                              int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out,
                              int num_rows_disp, int num_cols_disp, int elem_sz, float disp_scale,
                              int num_views, float angle, int num_disp, int zero_disp,
                              float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd,
                              int thresh_s, float thresh_h, int stages,
                              unsigned char *d_prev_img_l, unsigned char *d_prev_img_r, float *d_prev_disp_l, float *d_prev_disp_r,
                              float alpha, int thresh_color, float thresh_disp,
                              unsigned char *d_img_l, unsigned char *d_img_r);
/* The front of the reduced-resolution frame as a stage (an addition): from one side-by-side frame
 *   img_l, img_r      the two full-size split images, num_rows x num_cols x elem_sz (stm_d_demux_sbs's);
 *   low_l, low_r      the two reduced images, num_rows_disp x num_cols_disp x elem_sz: tx_scale_bilinear of img_l / img_r bit for bit
 *                     (the taps never cross from one eye into the other);
 *   census_l, _r      u32 planes of num_rows_disp x num_cols_disp: the low 32 bits of the reduced images' census transform, the word
 *                     the cost kernels read (window rows -1, +1, +2, +3; in a row x = -4 .. 4 without 0; MSB first).  Both null: not
 *                     returned.
 * Only the first three bytes of a pixel are written by the device flavour; the host flavour returns the bytes past the third as 0.
 * With num_cols_sbs >= 2 * num_cols all of it is one kernel launch (the same launch the reduced-resolution frame calls start with);
 * a narrower frame, and stm_set_agg_variant(600), run the chain of stages it replaces, with equal results.  Any sizes >= 1 are
 * legal, num_rows_disp >= num_rows included.  The _nv12_ calls take the NV12 planes of stm_demux_nv12 (its geometry rules, W =
 * num_cols) in place of the frame: the reduced images are tx_scale_bilinear of the converted split images.  Errors (stm_last_error),
 * all reported before anything is launched or written: a size < 1, elem_sz < 3, exactly one census plane null, the NV12 rules. */
void stm_demux_sbs_low(unsigned char *img_l, unsigned char *img_r, unsigned char *low_l, unsigned char *low_r,
                       unsigned int *census_l, unsigned int *census_r, unsigned char *img_sbs,
                       int num_rows, int num_cols_sbs, int num_cols, int num_rows_disp, int num_cols_disp, int elem_sz);
void stm_d_demux_sbs_low(unsigned char *d_img_l, unsigned char *d_img_r, unsigned char *d_low_l, unsigned char *d_low_r,
                         unsigned int *d_census_l, unsigned int *d_census_r, unsigned char *d_img_sbs,
                         int num_rows, int num_cols_sbs, int num_cols, int num_rows_disp, int num_cols_disp, int elem_sz);
void stm_demux_nv12_low(unsigned char *img_l, unsigned char *img_r, unsigned char *low_l, unsigned char *low_r,
                        unsigned int *census_l, unsigned int *census_r, unsigned char *y, int pitch_y, unsigned char *uv, int pitch_uv,
                        int num_rows, int num_cols_sbs, int num_cols, int num_rows_disp, int num_cols_disp, int elem_sz, int matrix);
void stm_d_demux_nv12_low(unsigned char *d_img_l, unsigned char *d_img_r, unsigned char *d_low_l, unsigned char *d_low_r,
                          unsigned int *d_census_l, unsigned int *d_census_r, unsigned char *d_y, int pitch_y, unsigned char *d_uv,
                          int pitch_uv, int num_rows, int num_cols_sbs, int num_cols, int num_rows_disp, int num_cols_disp, int elem_sz,
                          int matrix);
/* Guided disparity up-sampling (joint bilateral upsampling, Kopf et al. 2007; an addition: the reference's tx_disp_scale_kernel
 * blends four low-resolution values whatever the image shows, which smears every depth edge).  disp_low (f32, in_rows x in_cols)
 * is the map to scale up, img_low (u8, in_rows x in_cols x elem_sz) the image it was computed on, img (u8, out_rows x out_cols x
 * elem_sz) the guide; only the first three bytes of a pixel are read; all three are read only.  sigma_color must be > 0.
 *   tab[s] = (float)exp(-(double)(s * s) / (2.0 * (double)sigma_color * (double)sigma_color)),  s = 0 .. 765  (host, double, rounded once)
 * Per output pixel (x, y), f32 throughout, one operation per line, no contraction, C fmaxf / fminf / fabsf, correctly rounded
 * division; W, H = out_cols, out_rows and w, h = in_cols, in_rows:
 *   xs = ((float)x / (float)W) * (float)w;  xs = fminf(fmaxf(xs, 0), (float)(w - 1))          (tx_disp_scale's own mapping)
 *   ys = ((float)y / (float)H) * (float)h;  ys = fminf(fmaxf(ys, 0), (float)(h - 1))
 *   x0 = (int)floorf(xs);  y0 = (int)floorf(ys);  sw = 0;  swd = 0
 *   for j = -1, 0, 1, 2:  yi = y0 + j;  the row is skipped if yi < 0 or yi >= h
 *     wy = fmaxf(0, 1 - fabsf(ys - (float)yi) * 0.5f)
 *     for i = -1, 0, 1, 2:  xi = x0 + i;  the tap is skipped if xi < 0 or xi >= w
 *       wx  = fmaxf(0, 1 - fabsf(xs - (float)xi) * 0.5f)
 *       sad = |img[y][x][0] - img_low[yi][xi][0]| + |..[1] - ..[1]| + |..[2] - ..[2]|          (integer, 0 .. 765)
 *       wgt = (wy * wx) * tab[sad]
 *       sw  = sw + wgt
 *       t   = wgt * disp_low[yi][xi]
 *       swd = swd + t
 *   bil = what tx_disp_scale computes at (x, y) before its final multiplication (d_tx_scale.cu:8-28, d_alu.cu:17-43)
 *   out = (sw > 0 ? swd / sw : bil) * up
 * Taps outside the low-resolution image are skipped, not clamped.  In-image taps always take part, those of weight 0 included:
 * their 0 * inf is NaN, so non-finite values in disp_low spread as these lines say; sw itself is always finite.  Where no tap
 * resembles the guide pixel (sw == 0) the pixel is the plain bilinear value.  The 4 x 4 footprint is the same whatever the size
 * ratio; in_rows >= out_rows is legal.  Parity is against a numpy statement of these lines (parity unpinned). */
void stm_disp_upsample(float *disp_out, float *disp_low, unsigned char *img_low, unsigned char *img,
                       int out_rows, int out_cols, int in_rows, int in_cols, int elem_sz, float up, float sigma_color);
void stm_d_disp_upsample(float *d_disp_out, float *d_disp_low, unsigned char *d_img_low, unsigned char *d_img,
                         int out_rows, int out_cols, int in_rows, int in_cols, int elem_sz, float up, float sigma_color);
/* Temporal disparity stabilisation (an addition: the reference matches every frame of its video loop on its own, so on noisy
 * footage the maps, and with 0x200 / 0x800 the views, shimmer where nothing moves).  A motion-adaptive recursive filter on the
 * final maps, gated by how much the colour changed between two consecutive frames.  Inputs for one view:
 *   disp (cur)      f32 H x W: this frame's filtered map.  It is rewritten in place.
 *   disp_prev (prev) f32 H x W: the map that the previous frame output, which is that frame's filtered result.
 *   img, img_prev   u8 H x W x E, dense: the view's image in this frame and the previous one.  Only the first three bytes of a
 *                   pixel are read.  E = elem_sz >= 3.
 *   alpha           f32, the weight given to the history;  thresh_color  int;  thresh_disp  f32.
 *
 *   sad(q) = |img[q][0]-img_prev[q][0]| + |..[1]-..[1]| + |..[2]-..[2]|        (integer, 0..765)
 *   m(p)   = max of sad(q) over q = (x+i, y+j), i, j in {-1,0,1}, q inside the H x W image (clipped, not clamped)
 *   c = cur[p];  q = prev[p]
 *   t  = q - c
 *   df = fabsf(t)
 *   if (m(p) <= thresh_color && df <= thresh_disp) { u = alpha * t;  out = c + u; }   else out = c
 *
 * All arithmetic is f32, one operation per line, with no contraction.  A NaN in c or q makes the comparison false, so out = c.
 * An infinity behaves exactly as the lines say; with thresh_disp = +inf an infinite t passes the gate.
 * Argument rules: 0 <= alpha <= 1, 0 <= thresh_color <= 765, and thresh_disp >= 0 with +inf allowed.  Anything else, NaN
 * included, fails through stm_last_error before anything is launched or written.  prev must not alias cur (an error as well).
 * Parity is against a numpy statement of these lines (parity unpinned). */
void stm_disp_temporal(float *disp, float *disp_prev, unsigned char *img, unsigned char *img_prev, int num_rows, int num_cols,
                       int elem_sz, float alpha, int thresh_color, float thresh_disp);
void stm_d_disp_temporal(float *d_disp, float *d_disp_prev, unsigned char *d_img, unsigned char *d_img_prev, int num_rows, int num_cols,
                         int elem_sz, float alpha, int thresh_color, float thresh_disp);
/* The measurement behind the automatic depth budget (an addition; see stm_set_depth for what gain and conv do).  Both maps (f32,
 * num_rows x num_cols, read only) go into one histogram of 4096 quarter-pixel bins; per pixel, f32, one operation per line:
 *   v = disp * 4.0f
 *   v = fminf(fmaxf(v, -2048.0f), 2047.0f)          (C fmaxf: a NaN lands in bin 0; values beyond +-512 px land in the end bins)
 *   b = (int)floorf(v + 0.5f) + 2048
 * Every pixel of both maps counts once: n = 2 * num_rows * num_cols (u32; num_rows * num_cols must be below 2^31).
 *   k    = (u64)n * clip_permille / 1000
 *   lo   = the smallest b with cum(b) > k            (cum(b) = the count of bins 0 .. b)
 *   hi   = the largest b whose suffix count (bins b .. 4095) is > k          (clip_permille <= 499: lo <= hi always)
 *   d_lo = (float)(lo - 2048) * 0.25f;  d_hi = (float)(hi - 2048) * 0.25f
 * Then, in double, one operation per line, no contraction, correctly rounded division:
 *   span   = (double)d_hi - (double)d_lo
 *   budget = (double)disp_hi - (double)disp_lo
 *   g = span > 0 ? budget / span : max_gain
 *   g = min(g, max_gain)
 *   a = g * d_hi;  a = a - disp_hi                   (the least conv that brings the far end in)
 *   b = g * d_lo;  b = b - disp_lo                   (the most conv that keeps the near end in)
 *   c = min(max(0.0, a), b)
 * The minimal intervention: a scene that already fits [disp_lo, disp_hi] gets g = min(budget / span, max_gain) and c = 0.
 * state = four floats {valid, gain, conv, 0}.  valid == 0: the state becomes (1, (float)g, (float)c, 0).  Otherwise gain and conv
 * each move by rate, the other two floats stay:
 *   t = value - (double)old;  t = (double)rate * t;  new = (float)((double)old + t)
 * The device flavour reads and writes d_state in device memory and synchronises nothing; the host flavour takes and returns the
 * four floats in host memory.  Argument rules as stm_set_depth_auto; violations fail through stm_last_error before anything is
 * launched or written.  Parity is against a numpy statement of these lines (parity unpinned). */
void stm_depth_fit(float *disp_l, float *disp_r, int num_rows, int num_cols, float disp_lo, float disp_hi, float max_gain,
                   int clip_permille, float rate, float *state);
void stm_d_depth_fit(float *d_disp_l, float *d_disp_r, int num_rows, int num_cols, float disp_lo, float disp_hi, float max_gain,
                     int clip_permille, float rate, float *d_state);
/* The measurement behind the overlay's automatic depth placement (an addition; see stm_mux_overlay for what an overlay's disparity
 * does and stm_set_overlay_auto for the frame calls' use of it).  Inputs: the two maps of a frame (f32, num_rows x num_cols = H x W,
 * delta = x_right - x_left, read only); an overlay (ov_rows x ov_cols pixels B, G, R, A premultiplied, read only) at (x0, y0) in view
 * pixel space view_rows x view_cols = Hv x Wv (layout 0: the output frame; a quilt: one tile); the depth budget (gain, conv) = (g, c)
 * the frame is rendered with ((1, 0) without one); a state of four floats {valid, disparity, nearest, 0}.
 * 1. Alpha box.  r0 .. r1 and q0 .. q1 (inclusive) are the least and greatest overlay row and column holding a pixel with A != 0;
 *    none: n = 0.  (A mostly transparent full-width strip is not placed by what lies under its empty ends.)
 * 2. Footprint.  View rows [y0 + r0 - pad, y0 + r1 + 1 + pad) and columns [x0 + q0 - pad, x0 + q1 + 1 + pad), clipped to
 *    [0, Hv) x [0, Wv) = [ya, yb) x [xa, xb); in map pixels, 64-bit integers: rows [ya*H div Hv, (yb*H + Hv - 1) div Hv), columns
 *    [xa*W div Wv, (xb*W + Wv - 1) div Wv).  Empty: n = 0.  pad (view pixels) is the caller's allowance for the overlay's own
 *    parallax shift, the scene's warp between a map and a view, and breathing room; nothing else widens the footprint.
 * 3. Histogram.  Every pixel of BOTH maps inside the map rectangle into 4096 quarter-pixel bins by stm_depth_fit's line
 *      b = (int)floorf(fminf(fmaxf(4*disp, -2048), 2047) + 0.5f) + 2048
 *    except that a NaN is not counted (a NaN under a subtitle must not pull it to the near limit).  n = the pixels counted (u32).
 * 4. Nearest.  k = (u64)n * near_permille / 1000; lo = the first bin whose prefix count exceeds k; dp = (lo - 2048) * 0.25.
 *    (g >= 0, so the percentile commutes with the budget's map.)
 * 5. Target, in double, one operation per line, no contraction, correctly rounded division:
 *      e = g*dp;  e = e - c;  e = e * (double)Wv;  e = e / (double)W;  t = e - margin;  t = min(max(t, limit_lo), limit_hi)
 * 6. State.  n == 0: none of the four floats is written.  Otherwise the fit has no history when valid == 0, restart != 0, or a cut
 *    state is given (the 260 ints of stm_cut_detect) and its word 1, this frame's cut flag, is 1: then d = t.  With history:
 *      r = (t < d_old) ? rate_near : rate_far;  u = t - d_old;  u = r*u;  d = d_old + u;  d = min(max(d, limit_lo), limit_hi)
 *    and state = {1, (float)d, (float)e, 0}.  Two rates: a scene that comes nearer must be followed at once (rate_near is typically
 *    1) or the text collides with it; one that recedes is followed slowly, so that the text does not pump.  min and max are C's
 *    fmin and fmax: a NaN in the old state becomes limit_lo.
 * Smaller disparities are nearer (delta = x_right - x_left), so the near percentile is the low one and `nearest` is the displayed
 * disparity of the nearest scene content under the overlay, in view pixels.
 * The device flavour reads and writes d_state in device memory, reads d_cut_state (may be null) on the device and synchronises
 * nothing; the host flavour takes and returns the four floats in host memory.  Argument rules, violations fail through
 * stm_last_error before anything is launched or written: num_rows, num_cols, view_rows, view_cols >= 1 and num_rows * num_cols below
 * 2^31; the overlay's own as stm_mux_overlay's (the device flavour's pointer 4-byte aligned); gain in [0, 8] and |conv| <= 4096 as
 * stm_set_depth's; near_permille 0 .. 499; margin finite with |margin| <= 4096; pad 0 .. 4096; limit_lo <= limit_hi, both finite
 * with magnitude <= 4096; both rates in (0, 1].  Parity is against a numpy statement of these lines (parity unpinned). */
void stm_overlay_fit(float *disp_l, float *disp_r, int num_rows, int num_cols, const unsigned char *overlay, int ov_rows, int ov_cols, int x0,
                     int y0, int view_rows, int view_cols, float gain, float conv, int near_permille, float margin, int pad, float limit_lo,
                     float limit_hi, float rate_near, float rate_far, int restart, float *state);
void stm_d_overlay_fit(float *d_disp_l, float *d_disp_r, int num_rows, int num_cols, const unsigned char *d_overlay, int ov_rows, int ov_cols,
                       int x0, int y0, int view_rows, int view_cols, float gain, float conv, int near_permille, float margin, int pad,
                       float limit_lo, float limit_hi, float rate_near, float rate_far, int restart, float *d_state, const int *d_cut_state);
/* Vertical alignment as stages (an addition, see stm_set_align).  H = num_rows, W = num_cols of one unpacked eye.
 * stm_align_rows applies a field to one image (H x W x elem_sz, B G R first): out(y, x) = img sampled at row y + dy(x, y).
 * Per pixel -- f32, one operation per line, no contraction; then exact integers:
 *   u = (float)x - 0.5f * (float)(W - 1);  v = (float)y - 0.5f * (float)(H - 1)
 *   t = b * u;  s = a + t;  t = c * v;  s = s + t
 *   m = s * 16.0f;  m = m + 0.5f;  m = floorf(m);  m = fminf(fmaxf(m, -1024.0f), 1024.0f);  q = (int)m       (+-64 rows)
 *   y0 = y + (q >> 4);  f = q & 15                                                                 (arithmetic shift)
 *   out[ch] = ((16 - f) * img[clamp(y0)][x][ch] + f * img[clamp(y0 + 1)][x][ch] + 8) >> 4          ch = 0, 1, 2; rows clamp to [0, H-1]
 * f = 0 copies a row's pixel; a = b = c = 0 reproduces the image byte for byte.  Bytes of a pixel past the third: the device flavour
 * leaves them as they are in d_img_out, the host flavour returns them 0.  Rules: num_rows, num_cols >= 1, elem_sz >= 3, a, b, c
 * finite, no null pointer, img_out and img share no byte.
 *
 * stm_align_fit measures the field between two unpacked images.  KB = 8 column bands, band j = columns [j W / 8, (j+1) W / 8);
 * KR = 4 row blocks, block k = rows [k H / 4, (k+1) H / 4); R = radius; grey = (u8)(b*c + g*c + r*c), c = 0.33333334f, f32 one
 * operation per line (the grey of the census):
 *   1. P_e[j][y] = the sum of grey_e(y, x) over band j                                              u32, e = left, right
 *   2. G_e[j][y] = P_e[j][min(y+1, H-1)] - P_e[j][max(y-1, 0)]                                      i32 (a gradient: an exposure
 *                                                                                                   difference between the eyes cancels)
 *   3. S[j][k][d] = the sum over the rows y of block k of |G_L[j][y] - G_R[j][clamp(y + d, 0, H-1)]|, d = -R .. R      u32
 *      (at most 510 (W/8 + 1) (H/4 + 1): it fits 32 bits while (H/4 + 1) (W/8 + 1) <= 8421504, which is a rule of the call)
 *   4. per block i = j * 4 + k: the minimum of S over d, scanned d = 0, -1, +1, -2, +2, ... with strict less-than (ties go to the
 *      smaller |d|, then to the negative one).  The block is VALID iff the minimum is not at d = +-R and
 *      den = S[d-1] - 2 S[d] + S[d+1] > 0.  Then, in f64, one operation per line:
 *        t = (double)(S[d-1] - S[d+1]) / (double)den;  t = 0.5 * t;  o = (double)d + t
 *        t = (double)den * (double)(2R+1);  w = t / (double)max(1, the sum of S over d)
 *      with centre u_c = (x0 + x1 - 1) * 0.5 - (W - 1) * 0.5 of its band [x0, x1) and v_c likewise of its rows.
 *   5. the plane o ~ a + b u_c + c v_c by least squares over the blocks of weight > 0, a residual weighted by w (not w^2): the
 *      normal equations  M = sum w [1 u v]^T [1 u v],  r = sum w o [1 u v]^T  summed in block order i = 0 .. 31 and solved by
 *      Cramer's rule through the cofactors of M, f64, one operation per line, correctly rounded division (tests/test_align_ref.py's
 *      solve_ref states every line).  Fewer than 3 such blocks, or det(M) <= 1e-6 * M00 * M11 * M22 (the product of the diagonal
 *      bounds the determinant from above; a bare `det > 0` would let rounding decide for blocks of one band or one row block):
 *      b = c = 0 and a = r0 / M00, the weighted mean.  Then every block whose residual |o - (a + b u_c + c v_c)| exceeds 1.0
 *      loses its weight and the plane is solved once more over the rest (if nothing is left the first solution stands).
 *   6. state = four floats {valid, a, b, c}.  No valid block: the state is kept (one with valid == 0 becomes four zeros).
 *      Otherwise valid == 0: the state becomes (1, (float)a, (float)b, (float)c); else a, b, c each move by rate as stm_depth_fit's:
 *        t = value - (double)old;  t = (double)rate * t;  new = (float)((double)old + t)
 * The device flavour reads and writes d_state in device memory and synchronises nothing; d_valid_blocks (one int), d_profiles
 * (2 * 8 * num_rows words: P_left then P_right, [j][y]) and d_sad (8 * 4 * (2 radius + 1) words: [j][k][d + R]) receive what their
 * names say and may each be null.  The host flavour takes and returns the four floats in host memory and returns the number of
 * valid blocks (-1 on an error).  Rules: num_rows >= 4, num_cols >= 8, the size rule of step 3, elem_sz >= 3, radius in 1 .. 32, rate
 * in (0, 1], no null image or state.  Violations fail through stm_last_error before anything is launched or written.  Parity is
 * against the numpy statement of these lines in tests/test_align_ref.py (parity unpinned). */
void stm_align_rows(unsigned char *img_out, const unsigned char *img, int num_rows, int num_cols, int elem_sz, float a, float b, float c);
void stm_d_align_rows(unsigned char *d_img_out, const unsigned char *d_img, int num_rows, int num_cols, int elem_sz, float a, float b,
                      float c);
int  stm_align_fit(const unsigned char *img_l, const unsigned char *img_r, int num_rows, int num_cols, int elem_sz, int radius, float rate,
                   float *state);
void stm_d_align_fit(const unsigned char *d_img_l, const unsigned char *d_img_r, int num_rows, int num_cols, int elem_sz, int radius,
                     float rate, float *d_state, int *d_valid_blocks, unsigned int *d_profiles, unsigned int *d_sad);
/* Colour balance as stages (an addition, see stm_set_balance).  Everything is integer arithmetic, so the result depends on no order
 * of execution and no rounding mode.  N = H * W pixels of one unpacked eye; c is one of B, G, R; v, u, t are levels 0 .. 255.
 * stm_balance_fit:
 *   1. Histograms.  h[e][c][v], u32, over every pixel of eye e (0 = left, 1 = right); hist[(e * 3 + c) * 256 + v].  The calls
 *      refuse H * W >= 2^31.  From here on i64.
 *   2. Cumulative counts.  C[e][c][v] = sum of h[e][c][t] for t <= v.
 *   3. Mid-rank match.  m[c][v] = min{u : 2 C[0][c][u] >= 2 C[1][c][v] - h[1][c][v]}; the minimum exists because 2 C[0][c][255] = 2N.
 *      For two equal eyes m[v] = v at every occupied level.
 *   4. Offsets, smoothed over +-8 levels and weighted by the right eye's counts.  off[v] = m[v] - v; den[v] = the sum of h[1][c][t]
 *      over |t - v| <= 8, clipped to 0 .. 255; num[v] = the sum of h[1][c][t] * off[t] over the same range.  Where den[v] > 0:
 *      s[v] = floor((2 num[v] + den[v]) / (2 den[v])) -- floor division, which rounds half up for negative numerators as well (C's /
 *      truncates).  Where den[v] = 0: s[v] is the s of the nearest level BELOW v that has den > 0; if there is none, of the nearest
 *      above (one exists because N >= 1).
 *   5. Limit and order.  s[v] = clamp(s[v], -max_shift, max_shift); t[v] = clamp(v + s[v], 0, 255); then t[v] = max(t[v], t[v-1]) for
 *      v = 1 .. 255, so the table never inverts tones.
 *   6. State.  int32 state[769]: state[0] is the valid flag, state[1 + c * 256 + v] a level in 1/256 units.  With x = 256 t[v]: with no
 *      history (state[0] == 0) state = x and state[0] = 1; otherwise state += (rate_q * (x - state) + 128) >> 8, an arithmetic
 *      shift, with rate_q = clamp((int)floorf(rate * 256 + 0.5f), 1, 256) computed once on the host.  The update is
 *      non-decreasing in both state and x, so it keeps a monotone table monotone.
 * stm_balance_apply:
 *   7. lut[c][v] = clamp((state[1 + c*256 + v] + 128) >> 8, 0, 255) where a state is given, else the caller's 768 bytes (B, G, R, 256
 *      each, no monotonicity demanded).  out.c = lut[c][in.c] for the first three bytes of a pixel; the bytes past the third follow
 *      stm_align_rows' rules: the device flavour leaves them alone, the host flavour returns them 0.  img_out must not overlap img.
 * stm_d_balance_fit takes device pointers, synchronises nothing and writes the histograms into d_hist (1536 words) where it is not
 * null.  The host flavour takes and returns the 769 ints in host memory and returns 0 (-1 on an error).  stm_d_balance_apply takes
 * lut768 in HOST memory (it travels as a kernel argument) or d_state in device memory; the host flavour takes both in host memory.
 * Rules: num_rows, num_cols >= 1, num_rows * num_cols < 2^31, elem_sz >= 3, max_shift in 0 .. 255, rate in (0, 1], no null image or
 * state; for the apply calls exactly one of lut768 and state non-null.  Violations fail through stm_last_error before anything is
 * launched or written.  Parity is against the numpy statement of these lines in tests/test_balance_ref.py (parity unpinned). */
int  stm_balance_fit(const unsigned char *img_l, const unsigned char *img_r, int num_rows, int num_cols, int elem_sz, int max_shift,
                     float rate, int *state);
void stm_d_balance_fit(const unsigned char *d_img_l, const unsigned char *d_img_r, int num_rows, int num_cols, int elem_sz, int max_shift,
                       float rate, int *d_state, unsigned int *d_hist);
void stm_balance_apply(unsigned char *img_out, const unsigned char *img, int num_rows, int num_cols, int elem_sz,
                       const unsigned char *lut768, const int *state);
void stm_d_balance_apply(unsigned char *d_img_out, const unsigned char *d_img, int num_rows, int num_cols, int elem_sz,
                         const unsigned char *lut768, const int *d_state);
/* Shot changes as a stage (an addition, see stm_set_cut).  Everything is integer arithmetic; no result depends on the order of
 * execution.  The input is the LEFT eye of a frame, unpacked and converted as the other conditioning kernels see it: H x W pixels,
 * N = H * W.  The left eye is the reference of both the alignment and the balance, so the signature depends on neither.
 * State: int32 state[260] = {valid, cut, since, score, sig[256]}.
 *   1. Signature.  Y = (B + 2 G + R) >> 2; bin = Y >> 4; cell = ((4 y) / H) * 4 + (4 x) / W, a 4 x 4 grid, floor division;
 *      sig[cell * 16 + bin] counts the pixel, as u32.  The 256 counts sum to N.
 *   2. Score.  History exists when state[0] != 0 and the stored signature sums to N: a state left by a frame of another size counts as
 *      no history.  Without history score = 1000.  With history D = sum |sig[i] - old_sig[i]| in i64 (D <= 2N) and
 *      score = (1000 * D) / (2 * N), in 0 .. 1000.
 *   3. Decision.  since' = min(state[2] + 1, 2^30); cut = no history || (score >= thresh_permille && since' >= min_gap); then
 *      state = {1, cut, cut ? 0 : since', score, sig}.  The signature is stored on every frame, on a suppressed cut as well.
 *   4. Resets.  On a cut each non-null pointer of up to three receives one 32-bit zero: zero is the `valid` word of a float state and
 *      of an int state alike.  Otherwise the pointers are not touched.
 * stm_cut_detect takes the image in host memory and the state in and out, and returns the cut flag (-1 on an error).
 * stm_d_cut_detect takes device pointers, synchronises nothing and writes the signature into d_sig (256 words) where it is not null.
 * Rules: num_rows, num_cols >= 4 (no cell is empty), num_rows * num_cols < 2^31, elem_sz >= 3, thresh_permille in 1 .. 1000,
 * min_gap in 1 .. 2^20 (1: any frame may be a cut; larger values keep a photographer's flash from being two cuts), no null image
 * or state.  Violations fail through stm_last_error before anything is launched or written.  Known limits: dissolves and fades
 * are not cuts; a global exposure step of about 16 levels can score as one.  Parity is against the numpy statement of these lines in
 * tests/test_cut_ref.py (parity unpinned). */
int  stm_cut_detect(const unsigned char *img_l, int num_rows, int num_cols, int elem_sz, int thresh_permille, int min_gap, int *state);
void stm_d_cut_detect(const unsigned char *d_img_l, int num_rows, int num_cols, int elem_sz, int thresh_permille, int min_gap, int *d_state,
                      void *d_reset0, void *d_reset1, void *d_reset2, unsigned int *d_sig);
/* The active picture area as stages (an addition, see stm_set_active).  Everything is integer arithmetic; no result depends on the
 * order of execution.  The input is the LEFT eye of a frame, unpacked and converted as the shot-change detector sees it: H x W pixels.
 * State: int32 state[16] = {valid, top, bottom, left, right, changed, H, W, cand[4], run[4]}; the four sides are numbered top, bottom,
 * left, right.
 *   1. Lit pixels.  Y = (B + 2 G + R) >> 2 (stm_cut_detect's luma); a pixel is lit when Y > thresh_luma.
 *   2. Counts.  r[y] = the lit pixels of row y, c[x] = the lit pixels of column x, u32; counts = r then c, H + W words.
 *   3. Picture lines, in u64.  Row y is a picture row when r[y] * 1000 > lit_permille * W; column x is a picture column when
 *      c[x] * 1000 > lit_permille * H (the column's count runs over all rows, the bars' included).  A burnt-in logo or a few hot
 *      pixels in a bar stay below the permille and move nothing.
 *   4. Bars of this frame.  m[0] = the rows above the first picture row, m[1] = the rows below the last, m[2], m[3] likewise for the
 *      columns left of the first and right of the last picture column.  No picture row or no picture column: the frame is BLANK.
 *      Otherwise m[0], m[1] = min(m, H * max_bar_permille / 1000) and m[2], m[3] = min(m, W * max_bar_permille / 1000), floor
 *      division: at most 450 permille a side, so the rectangle is never empty and a night scene with a lit centre cannot turn most
 *      of the frame into bars.
 *   5. History exists when state[0] != 0, state[6] == H and state[7] == W: a state left by a frame of another size counts as none.
 *      The fit RESTARTS when there is no history, when restart != 0, or when a cut state is given (the 260 ints of stm_cut_detect)
 *      and its word 1, this frame's cut flag, is 1.
 *   6. Blank frame.  With history and no restart only `changed` is written, as 0: a fade through black says nothing.  Otherwise the
 *      state becomes {0, 0, H, 0, W, 0, H, W, 0 x 8}: no bars, nothing known, the next frame that is not blank starts afresh.
 *   7. Otherwise, each side i on its own, b = m[i], B = the bar the state holds (top, H - bottom, left, W - right; 0 without history):
 *        on a restart      B = b, cand = b, run = 0
 *        b <  B            B = b, run = 0                      (picture was seen inside the bar: it is given back at once)
 *        b == B            run = 0
 *        b >  B            cand = (run == 0) ? b : min(cand, b);  run += 1;  if run >= hold: B = cand, run = 0
 *      so a bar grows only after `hold` consecutive frames that agree on at least that much, and to the least of them; hold = 1
 *      takes every frame on its own.  state = {1, B0, H - B1, B2, W - B3, changed, H, W, cand, run}; changed = 1 when the rectangle
 *      differs from the one the state held (the whole frame, without history), else 0.
 * The rectangle is rows [top, bottom) and columns [left, right): the state's words 1 .. 4, which is what every consumer below takes
 * as four ints in device memory.
 * stm_active_detect takes the image in host memory and the state in and out, and returns `changed` (-1 on an error).
 * stm_d_active_detect takes device pointers, synchronises nothing, reads d_cut_state (may be null) on the device and writes the
 * counts into d_counts (H + W words, rows first) where it is not null.
 * Rules: num_rows, num_cols >= 1, num_rows * num_cols < 2^31, elem_sz >= 3, thresh_luma in 0 .. 254, lit_permille in 0 .. 999,
 * max_bar_permille in 0 .. 450, hold in 1 .. 2^20, no null image or state.  Violations fail through stm_last_error before anything is
 * launched or written.  Parity is against the numpy statement of these lines in tests/test_active_ref.py (parity unpinned).
 *
 * stm_active_fill: every pixel of disp (f32, num_rows x num_cols) outside the rectangle becomes `value`, bit for bit; the pixels
 * inside are not touched, NaNs included.  One launch that visits the four strips only; a full rectangle writes nothing, and so does
 * a null one.  The device flavour reads the four ints on the device, clamped to the map (no store can leave it), the host flavour
 * takes four host ints under the rule 0 <= top < bottom <= num_rows, 0 <= left < right <= num_cols.
 *
 * stm_depth_fit_rect is stm_depth_fit with only the pixels of both maps inside the rectangle counted, so n = twice its area; a null
 * rectangle is stm_depth_fit itself, launch for launch.  stm_overlay_fit_rect is stm_overlay_fit with one line after step 2: the map
 * rectangle is moved into the active one, per axis, with [a, b) the footprint's interval and [A, B) the active one:
 *      if max(a, A) < min(b, B): [max(a, A), min(b, B));  else len = min(b - a, B - A) and [A, A + len) where b <= A, [B - len, B)
 *      where a >= B
 * so a subtitle that lies wholly in the bottom bar is placed by the picture rows nearest to it, not left unplaced.  Steps 3 to 6 are
 * unchanged; a null rectangle is stm_overlay_fit itself.  In both, the device flavour takes the rectangle in device memory (clamped
 * to the map as above), the host flavour four host ints under stm_active_fill's rule. */
int  stm_active_detect(const unsigned char *img_l, int num_rows, int num_cols, int elem_sz, int thresh_luma, int lit_permille,
                       int max_bar_permille, int hold, int restart, int *state);
void stm_d_active_detect(const unsigned char *d_img_l, int num_rows, int num_cols, int elem_sz, int thresh_luma, int lit_permille,
                         int max_bar_permille, int hold, int restart, int *d_state, const int *d_cut_state, unsigned int *d_counts);
void stm_active_fill(float *disp, int num_rows, int num_cols, const int *rect, float value);
void stm_d_active_fill(float *d_disp, int num_rows, int num_cols, const int *d_rect, float value);
void stm_depth_fit_rect(float *disp_l, float *disp_r, int num_rows, int num_cols, float disp_lo, float disp_hi, float max_gain,
                        int clip_permille, float rate, float *state, const int *rect);
void stm_d_depth_fit_rect(float *d_disp_l, float *d_disp_r, int num_rows, int num_cols, float disp_lo, float disp_hi, float max_gain,
                          int clip_permille, float rate, float *d_state, const int *d_rect);
void stm_overlay_fit_rect(float *disp_l, float *disp_r, int num_rows, int num_cols, const unsigned char *overlay, int ov_rows, int ov_cols,
                          int x0, int y0, int view_rows, int view_cols, float gain, float conv, int near_permille, float margin, int pad,
                          float limit_lo, float limit_hi, float rate_near, float rate_far, int restart, float *state, const int *rect);
void stm_d_overlay_fit_rect(float *d_disp_l, float *d_disp_r, int num_rows, int num_cols, const unsigned char *d_overlay, int ov_rows,
                            int ov_cols, int x0, int y0, int view_rows, int view_cols, float gain, float conv, int near_permille, float margin,
                            int pad, float limit_lo, float limit_hi, float rate_near, float rate_far, int restart, float *d_state,
                            const int *d_cut_state, const int *d_rect);
/* View antialiasing: the depth-adaptive prefilter of one image by its own map (an addition, the reference has none: each of its views
 * is a pinhole image at one camera position s, while a lenticular lens shows a band about one view spacing wide.  A scene point of
 * displayed end-to-end disparity e moves e / (N - 1) pixels between adjacent views, so detail finer than that step aliases between
 * views: doubled edges, crawling texture).  For locally constant depth the band limit along the view axis is a horizontal box blur
 * whose width grows with the pixel's displayed disparity.  img (num_rows x num_cols x elem_sz, B G R first) is filtered by disp (f32,
 * num_rows x num_cols, delta = d - zero_disp): the left image by disp_l, the right image by disp_r.  img_out must not overlap img.
 * Per pixel x of a row -- f32, one operation per line, no contraction, C fabsf / fminf:
 *   k16 = (float)((double)strength * 8.0 / (double)(num_views - 1))                                  (host, once)
 *   p = gain * delta[x];  e = p - conv;  a = fabsf(e)           (e: the displayed disparity, stm_set_depth's gain * delta - conv)
 *   H = 0 if a is not finite, else (int)(fminf(a * k16, (float)(16 * max_radius)) + 0.5f)            per-side extension in 1/16 px
 *   K = (H + 15) >> 4
 *   for k = 1 .. K:  w_k = min(16, H - 16 * (k - 1))
 *       for j in (x - k, x + k):  jc = clamp(j, 0, num_cols - 1)
 *           the tap jc is USED iff fabsf(delta[jc] - delta[x]) <= gate                               (false for NaN)
 *   T      = 16 + the sum of the used taps' w_k
 *   out[c] = (16 * img[x][c] + the sum of the used w_k * img[jc][c] + (T >> 1)) / T                  integer division, c = 0, 1, 2
 * H = 0 copies the pixel: content on the displayed screen plane is byte-identical.  With every tap used the box is
 * 1 + strength * |e| / (N - 1) pixels wide in all -- continuous at 0, and it never sharpens.  The gate keeps a blurred pixel from
 * pulling in colours across a depth edge (the usual leak of a gather blur).  T <= 528 and every numerator <= 255 * 528 + 264.
 * Bytes of a pixel past the third: the device flavour leaves them as they are in d_img_out, the host flavour returns them 0.
 * Argument rules: num_rows, num_cols >= 1, elem_sz >= 3, num_views >= 2; strength finite in [0, 8]; max_radius in 1 .. 16; gate finite
 * and >= 0; gain, conv by stm_set_depth's mode-1 rules; no null pointer; img_out and img share no byte.  Violations fail through
 * stm_last_error before anything is launched or written.  Parity is against a numpy statement of these lines (parity unpinned). */
void stm_view_prefilter(unsigned char *img_out, const unsigned char *img, const float *disp, int num_rows, int num_cols, int elem_sz,
                        int num_views, float strength, int max_radius, float gate, float gain, float conv);
void stm_d_view_prefilter(unsigned char *d_img_out, const unsigned char *d_img, const float *d_disp, int num_rows, int num_cols,
                          int elem_sz, int num_views, float strength, int max_radius, float gate, float gain, float conv);
/* d_tx_scale.h:17-18  d_tx_scale (d_tx_scale.cu:83-121): bilinear image resize; HOST pointers despite the name */
void stm_d_tx_scale(unsigned char *img_in, unsigned char *img_out, int in_rows, int in_cols, int out_rows, int out_cols,
                    int elem_sz);

/* d_filter_gaussian.h:30 (d_filter_gaussian.cu:237-255): the (2r+1)^2 spatial kernel the two big stencils use,
 * exp(-(x^2+y^2)/(2 s^2)) / (2 pi s^2) with the reference's float/double mix, row-major.  Host-only helper. */
void stm_generate_gaussian_kernel(float *kernel, int radius, float sigma);

/* ------------------------------------------------- frame sequences */
/* The reference's video loop (video_io.cpp:144-165) calls adcensus_stm once per decoded frame, serialising upload,
 * compute and download.  A frame stream keeps the same per-frame contract (one side-by-side frame in; disp_l,
 * disp_r and the interlaced frame out, in submission order) over double-buffered pinned/device buffers and three
 * HIP streams, so frame k+1 uploads and frame k-1 downloads while frame k computes.  From its third frame on each
 * buffer slot replays the frame's kernel launches as a captured hipGraph (environment STM_STREAM_GRAPH=0 turns
 * that off).  A stream belongs to the host thread that created it.  Parameters as adcensus_stm. */
void *stm_stream_create(int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out, int elem_sz,
                        int num_views, float angle, int num_disp, int zero_disp, float ad_coeff, float census_coeff,
                        float ucd, float lcd, int usd, int lsd, int thresh_s, float thresh_h);
/* stages the next frame (the caller's buffer is reusable on return); at most two frames in flight.
 * Returns the frame index, or -1 if both slots are uncollected. */
long  stm_stream_submit(void *stream, const unsigned char *img_sbs);
/* the `stages` word the stream's frames are computed with: 3 (the default), optionally OR-ed with 0x200, 0x400, 0x800 and / or
 * 0x2000 (not 0x100; 0x1000 only after stm_stream_set_match_size).  With 0x2000 every frame but the first is an stm_d_adcensus_stm_t call whose history is the
 * frame before it (its input and its stabilised maps, which stay in the stream's other buffer slot); the two frames in flight
 * then run one after the other on the GPU, while upload and download still overlap.  A history reset at a scene cut is not
 * offered: the colour gate refuses to blend across one.  Only before the first submit.  Returns 0, or -1 with stm_last_error set. */
int   stm_stream_set_stages(void *stream, int stages);
/* the size every frame of the stream is matched at: with num_rows_disp x num_cols_disp set, a frame is the reduced-resolution frame
 * with this disp_scale -- an stm_d_adcensus_stm_2s call, stm_d_adcensus_stm_2t with 0x2000 in the stream's stages, or
 * stm_d_adcensus_stm_2nv12 in NV12 mode, picked as the full-resolution calls are -- and stm_stream_set_stages also accepts 0x1000.
 * (0, 0, any) = off, the default.  Otherwise both sizes must be >= 1 and disp_scale finite and > 0.  Lens, layout and depth reach the
 * reduced frame's render as they reach the full-resolution one.  Errors: after the first submit; together with a packing of the
 * stream, in whichever order the two setters are called; switching it off while the stream's stages hold 0x1000.  Returns 0, or -1
 * with stm_last_error set and the stream unchanged. */
int   stm_stream_set_match_size(void *stream, int num_rows_disp, int num_cols_disp, float disp_scale);
/* the parameters of the temporal step of a stream whose stages carry 0x2000 (stm_disp_temporal's rules; defaults 0.5, 24, 1.5).
 * Only before the first submit.  Returns 0, or -1 with stm_last_error set. */
int   stm_stream_set_temporal(void *stream, float alpha, int thresh_color, float thresh_disp);
/* the input format of the stream's frames: 0 = one side-by-side BGR frame (the default), 1 = NV12 with conversion `matrix`
 * (stm_demux_nv12's rules: num_rows and num_cols even, num_cols_sbs even and >= 2 * num_cols; elem_sz as created).  In NV12 mode a
 * frame is the Y plane (pitch num_cols_sbs) followed by the UV plane at byte num_rows * num_cols_sbs (pitch num_cols_sbs):
 * stm_stream_submit reads, and stm_stream_input_buffer hands out, num_rows * num_cols_sbs * 3 / 2 bytes in that layout, and half
 * the bytes of a BGR frame cross the link.  Every frame is an stm_d_adcensus_stm_nv12 call; each buffer slot owns its two split
 * images, and with 0x2000 the other slot's images and maps are the history.  `matrix` is ignored for format 0.  Only before the
 * first submit.  Returns 0, or -1 with stm_last_error set. */
int   stm_stream_set_input(void *stream, int format, int matrix);
/* the packing of the stream's input frames (stm_set_packing's settings; the geometry rules of stm_demux_packed, in NV12 mode those of
 * stm_demux_nv12_packed, on the stream's num_rows, num_cols_sbs and num_cols with both pitches num_cols_sbs; the default is
 * (0, 0, 0, 0)).  num_rows and num_cols stay the unpacked eye's size; a frame then has rows_f rows of num_cols_sbs pixels:
 * stm_stream_submit reads rows_f * num_cols_sbs * elem_sz bytes, in NV12 mode rows_f * num_cols_sbs * 3 / 2 (the UV plane at byte
 * rows_f * num_cols_sbs), so a half packing uploads half the bytes again.  Each slot's pinned and device input buffers are allocated
 * anew for rows_f * num_cols_sbs * elem_sz bytes: pointers obtained from stm_stream_input_buffer BEFORE this call are void afterwards.
 * It combines with stm_stream_set_input in either order (whichever comes second checks the combination), with 0x2000 (in BGR mode the
 * other slot's packed frame is the history, unpacked by one extra launch) and with the captured graphs: the gather reads nothing back.
 * The stream keeps its own copy and installs it only around its frame calls, like the lens geometry.  Only before the first submit.
 * Returns 0, or -1 with stm_last_error set and the stream unchanged. */
int   stm_stream_set_packing(void *stream, int packing, int swap, int filter, int gap);
/* the display geometry of the stream's frames (stm_set_lens's rules; the default is mode 0).  The stream keeps its own copy and
 * installs it only for the duration of its frame calls: the calling thread's stm_set_lens neither reaches the stream's frames
 * (or its captured graph) nor is changed by them.  Only before the first submit.  Returns 0, or -1 with stm_last_error set. */
int   stm_stream_set_lens(void *stream, int mode, double pitch, double slope, double centre);
/* the output geometry of the stream's frames (stm_set_layout's rules; the default is layout 0).  The stream keeps its own copy and
 * installs it only for the duration of its frame calls, like the lens geometry: the calling thread's stm_set_layout neither reaches
 * the stream's frames nor is changed by them.  Only before the first submit.  Returns 0, or -1 with the error recorded. */
int   stm_stream_set_layout(void *stream, int layout, int tiles_x, int tiles_y, int order, int filter);
/* the output format of the stream's frames (stm_set_output's formats and matrices; the default is format 0).  Format 1: every frame
 * leaves as one contiguous NV12 surface, P = num_cols_out and R = num_rows_out, as the stream's NV12 input is contiguous; the output
 * size becomes num_rows_out * num_cols_out * 3 / 2 bytes: what stm_stream_collect copies, what the download moves and what
 * stm_stream_collect_view points at.  The stream keeps its own copy and installs it only around its frame calls, like the layout.
 * Refused while the stream's layout is 0, and stm_stream_set_layout(stream, 0, ...) is refused while the format is 1; refused as well
 * while the stream has an overlay (stm_stream_set_overlay), which in turn is refused while the format is 1.  It replays
 * under the captured graphs (nothing is read back) and combines with every input format, packing, match size, 0x2000 and depth mode.
 * Only before the first submit.  Returns 0, or -1 with stm_last_error set and the stream unchanged. */
int   stm_stream_set_output(void *stream, int format, int matrix);
/* the overlay of the stream's frames (stm_mux_overlay's definition, under the stream's own lens and layout).
 * stm_stream_set_overlay(stream, max_rows, max_cols) switches it on for overlays of up to max_rows x max_cols pixels (both in
 * 1 .. 65535; (0, 0) = off, the default) and allocates a pinned and a device copy per buffer slot.  Only before the first submit.
 * Refused while the stream's output format is 1 (NV12), and stm_stream_set_output(stream, 1, ...) is refused while it is on.
 * stm_stream_overlay sets the overlay every LATER submit composites, until the next call: host memory, ov_rows x ov_cols x 4 bytes,
 * reusable on return; NULL or a zero size = no overlay (the other arguments are then ignored).  It may be called between any two
 * submits (subtitles change): frame k shows exactly the overlay in force when it was submitted.  That holds with the captured graphs
 * on: a slot whose device copy is stale uploads it on the upload stream ahead of the frame, and the composite is launched on the slot's
 * compute stream after the frame's graph (or its eager pipeline) and before the frame counts as done, so its arguments are never baked
 * into a graph.  The maps, and with 0x2000 the history, never see the overlay.  The calling thread's stm_set_overlay neither reaches
 * a stream's frames nor is changed by them.  Errors (stm_last_error, the stream unchanged): stm_mux_overlay's rules for the overlay's
 * own arguments (its pointer may have any alignment here); an overlay larger than max_rows x max_cols; stm_stream_overlay on a stream
 * without stm_stream_set_overlay.  Return 0, or -1 with stm_last_error set. */
int   stm_stream_set_overlay(void *stream, int max_rows, int max_cols);
int   stm_stream_overlay(void *stream, const unsigned char *overlay, int ov_rows, int ov_cols, int x0, int y0, float disparity);
/* the automatic placement of the stream's overlay (stm_set_overlay_auto's definition and rules, under the stream's own lens, layout,
 * depth budget and cut detector).  Accepted only before the first submit and after stm_stream_set_overlay (switching that off
 * switches this off too).  The state is the stream's own, 16 bytes at a fixed address zeroed when it is allocated; the fit and the
 * compositor are launched behind the slot's captured graph, where the overlay is composited, so their arguments change from submit
 * to submit.  Frame k reads the state frame k - 1 left (its compute waits for the other slot's frame, as depth mode 2 arranges
 * it).  A submit whose overlay comes from another stm_stream_overlay call than the previously fitted frame's passes restart = 1: a
 * new subtitle has no continuity to keep.  stm_stream_overlay's disparity is then ignored.
 * stm_stream_overlay_depth reports the four floats as the most recently collected frame left them (with the placement off:
 * {0, the disparity that frame was submitted under, 0, 0}); -1 before the first collect.  Return 0, or -1 with stm_last_error set. */
int   stm_stream_set_overlay_auto(void *stream, int mode, int near_permille, float margin, int pad, float limit_lo, float limit_hi,
                                  float rate_near, float rate_far);
int   stm_stream_overlay_depth(void *stream, float out[4]);
/* the depth budget of the stream's frames (stm_set_depth's rules; the default is mode 0).  As with the lens geometry the stream keeps
 * its own copy and installs it only around its frame calls.  stm_stream_set_depth_auto sets mode 2's parameters (stm_set_depth_auto's
 * rules; call it before stm_stream_set_depth(stream, 2, 0, 0)); the state is the stream's own: one buffer at a fixed address, zeroed
 * at creation, so the slots' captured graphs stay valid.  Frame k reads what frame k - 1 wrote, so in mode 2 the two frames in
 * flight run one after the other on the GPU, as with 0x2000; upload and download still overlap.  Only before the first submit.
 * Return 0, or -1 with stm_last_error set. */
int   stm_stream_set_depth(void *stream, int mode, float gain, float conv);
int   stm_stream_set_depth_auto(void *stream, float disp_lo, float disp_hi, float max_gain, int clip_permille, float rate);
/* the view antialiasing of the stream's frames (stm_set_antialias's rules; the default is mode 0).  As with the depth budget the
 * stream keeps its own copy and installs it only around its frame calls, so the prefilter is part of the slots' captured graphs and
 * replays with them.  Only before the first submit.  Returns 0, or -1 with stm_last_error set and the stream unchanged. */
int   stm_stream_set_antialias(void *stream, int mode, float strength, int max_radius, float gate);
/* out = {gain, conv} applied to the most recently collected frame: in mode 2 the state as that frame's fit left it (a 16-byte copy
 * taken on the frame's compute stream and downloaded with its results, so the next frame's update cannot race it), in mode 1 the
 * setting, in mode 0 {1, 0}.  Returns 0, or -1 if no frame has been collected yet. */
int   stm_stream_depth(void *stream, float out[2]);
/* the vertical alignment of the stream's frames (stm_set_align's rules; the default is mode 0, and the calling thread's own setting
 * never reaches a stream's frames).  The stream keeps its own copy and installs it only around its frame calls, so the measurement
 * and the kernel that applies the field are part of the slots' captured graphs.  stm_stream_set_align_auto sets mode 2's radius and
 * rate (stm_set_align_auto's rules; the defaults are 16 and 1); the state is the stream's own: one buffer at a fixed address, zeroed
 * when mode 2 is first set.  Frame k reads what frame k - 1 wrote, so in mode 2 the two frames in flight run one after the other
 * on the GPU, as with depth mode 2.  Mode 2 needs stm_set_align's size rules on the stream's geometry.  Only before the first
 * submit.  Return 0, or -1 with stm_last_error set and the stream unchanged. */
int   stm_stream_set_align(void *stream, int mode, float a, float b, float c);
int   stm_stream_set_align_auto(void *stream, int radius, float rate);
/* out = {a, b, c} applied to the most recently collected frame: in mode 2 the state as that frame's fit left it (copied and
 * downloaded as stm_stream_depth's), in mode 1 the setting, in mode 0 zeros.  Returns 0, or -1 if no frame has been collected yet. */
int   stm_stream_align(void *stream, float out[3]);
/* the colour balance of the stream's frames (stm_set_balance's rules; the default is mode 0, and the calling thread's own setting
 * never reaches a stream's frames).  Kept and installed like the alignment.  stm_stream_set_balance_auto sets mode 2's max_shift
 * and rate (stm_set_balance_auto's rules; the defaults are 48 and 1); the state is the stream's own: one buffer at a fixed
 * address, zeroed when mode 2 is first set.  Frame k reads what frame k - 1 wrote, so in mode 2 the two frames in flight run one
 * after the other on the GPU, as with depth mode 2 and alignment mode 2.  Only before the first submit.  Return 0, or -1 with
 * stm_last_error set and the stream unchanged. */
int   stm_stream_set_balance(void *stream, int mode, const unsigned char *lut768);
int   stm_stream_set_balance_auto(void *stream, int max_shift, float rate);
/* out_lut = the 768 bytes applied to the most recently collected frame: in mode 2 step 7's tables of the state as that frame's fit
 * left it (copied per slot and downloaded with the results), in mode 1 the setting, in mode 0 the identity.  Returns 0, or -1 if
 * no frame has been collected yet. */
int   stm_stream_balance(void *stream, unsigned char out_lut[768]);
/* the shot-change detector of the stream's frames (stm_set_cut's rules; the default is mode 0, and the calling thread's own setting
 * never reaches a stream's frames).  The state is the stream's own: one buffer at a fixed address, zeroed when mode 1 is first set,
 * so the slots' captured graphs stay valid.  The reset pointers are the stream's own depth, alignment and balance states, for those
 * whose mode is 2; they are resolved at submit, so the setters may come in any order.  Frame k reads what frame k - 1 wrote, so with
 * mode 1 the two frames in flight run one after the other on the GPU, as with depth mode 2.  Only before the first submit.  Returns
 * 0, or -1 with stm_last_error set and the stream unchanged. */
int   stm_stream_set_cut(void *stream, int mode, int thresh_permille, int min_gap);
/* out = {cut, score, since} of the most recently collected frame (12 bytes copied per slot after the decision and downloaded with
 * the results, as stm_stream_depth's); in mode 0 {0, 0, 0}.  Returns 0, or -1 if no frame has been collected yet. */
int   stm_stream_cut(void *stream, int out[3]);
/* the active picture area of the stream's frames (stm_set_active's and stm_set_active_auto's rules in one call; the default is mode
 * 0, and the calling thread's own setting never reaches a stream's frames).  Mode 1's rectangle is screened against the stream's
 * num_rows x num_cols here.  The state is the stream's own: 16 ints at a fixed address, zeroed when mode 2 is set, so the slots'
 * captured graphs stay valid and replay the measurement, the fill and both fits.  The cut state mode 2 reads is the stream's own
 * (stm_stream_set_cut); it is resolved at submit, so the setters may come in any order.  Frame k reads what frame k - 1 wrote, so
 * with mode 2 the two frames in flight run one after the other on the GPU, as with the cut detector.  The stream's automatic overlay
 * placement (stm_stream_set_overlay_auto) is fitted under the rectangle in modes 1 and 2.  Only before the first submit.  Returns 0,
 * or -1 with stm_last_error set and the stream unchanged. */
int   stm_stream_set_active(void *stream, int mode, const int rect[4], int fill, float fill_disp, int thresh_luma, int lit_permille,
                            int max_bar_permille, int hold);
/* out = {top, bottom, left, right, changed} of the most recently collected frame (20 bytes copied per slot after the decision and
 * downloaded with the results, as stm_stream_cut's); in mode 1 the given rectangle and 0, in mode 0 the whole frame and 0.  Returns
 * 0, or -1 if no frame has been collected yet. */
int   stm_stream_active(void *stream, int out[5]);
/* waits for the oldest uncollected frame and copies its results out (NULL = skip).  Returns its index or -1. */
long  stm_stream_collect(void *stream, float *disp_l, float *disp_r, unsigned char *interlaced);
/* zero-copy variants (at 1080p the two host copies of submit / collect take longer than the frame does on the GPU):
 * the pinned input buffer of the slot the next submit will use (NULL while that slot is uncollected) -- write the frame
 * into it and pass the same pointer (or NULL) to stm_stream_submit; and a collect that hands out pointers to the pinned
 * result buffers, valid until the frame after the next one is submitted. */
unsigned char *stm_stream_input_buffer(void *stream);
long  stm_stream_collect_view(void *stream, const float **disp_l, const float **disp_r, const unsigned char **interlaced);
/* what a frame's two disparity maps leave the stream as.  An addition: the reference's loop hands out float maps only, and at 1080p
 * they are 16.6 of the 22.8 MB a frame downloads.
 *   format 0 = float32 maps, the default: exactly the stream without this call;  1 = no maps;  2 = u8 planes;  3 = u16 planes.
 *   which (formats 2 and 3; ignored otherwise): 0 = the left map only, 1 = the right map only, 2 = both.
 *   lo, hi (formats 2 and 3; ignored otherwise): the map values that code 0 and code maxcode stand for.
 * Definition of a plane, f32, one operation per line, for a map value d and maxcode = 255 (u8) or 65535 (u16):
 *   k    = (float)((double)maxcode / ((double)hi - (double)lo))    on the host, once; negative when hi < lo, so either of
 *                                                                   near = bright and near = dark is a choice of lo and hi
 *   t    = d - lo
 *   t    = t * k                                                   (two roundings: no fused multiply-add)
 *   t    = fmaxf(t, 0.0f)                                          (a NaN becomes 0: fmaxf returns its other operand)
 *   t    = fminf(t, (float)maxcode)
 *   code = (unsigned)(t + 0.5f)                                    (exact: t + 0.5 <= 65535.5 is an f32)
 * A stream's maps are always finite; the NaN rule only makes the definition total.  A plane is tight: num_rows rows of num_cols
 * codes with no pitch, the rows x cols of the float maps the stream hands out in format 0 -- for a stream with a match size too,
 * whose maps are full-resolution.  u16 codes are little-endian.
 * With a format other than 0 the float maps are still computed, and stay on the device: 0x2000's history, the renderer and the
 * overlay fit read them as before, and the interlaced frames are byte for byte those of format 0.  The two float downloads are
 * not issued and their pinned buffers not held.  Formats 2 and 3 hold a device and a pinned buffer per slot for the planes (the
 * selected ones, tight behind each other); one kernel launch per frame quantises them on the slot's compute stream right behind
 * the frame -- inside the slot's captured graph, its arguments being fixed -- and they are downloaded with the frame.
 * stm_stream_collect and stm_stream_collect_view then refuse a non-null map pointer (-1, stm_last_error set, nothing consumed:
 * the frame can still be collected) and work as before with both null.  stm_stream_collect_maps and stm_stream_collect_maps_view
 * are their counterparts for formats 1 to 3: plane_l / plane_r receive (or point at) num_rows * num_cols codes of 1 or 2 bytes.
 * A plane the stream does not produce -- not selected by `which`, or any plane in format 1 -- has a NULL view, and a non-null
 * destination for it is refused like a map pointer above; on a stream of format 0 both calls are refused.  The views stay valid
 * until the frame after the next one is submitted.  Every other setting of the stream combines with every format.
 * stm_stream_maps errors (stm_last_error names stream_maps; -1, the stream unchanged): a format outside 0 .. 3; for formats 2 and 3
 * a `which` outside 0 .. 2, lo or hi not finite or beyond +-4096, |hi - lo| < 1/64; a call after the first submit.  Returns 0. */
int   stm_stream_maps(void *stream, int format, int which, float lo, float hi);
long  stm_stream_collect_maps(void *stream, void *plane_l, void *plane_r, unsigned char *interlaced);
long  stm_stream_collect_maps_view(void *stream, const void **plane_l, const void **plane_r, const unsigned char **interlaced);
/* image-plus-depth input of a frame stream (an image with its depth plane in, the second eye built on the GPU): its one entry
 * point is declared, with the definition line by line, in stm_depth_input.h.  This header's set of names is recorded in the
 * screening tables of the test suite and stays what it is.
 * Rectification from camera calibration (both eyes remapped through a camera matrix, distortion coefficients and a rectifying
 * rotation, as a stage and as the first step of a stream's frames): its entry points are declared, with the definition line by
 * line, in stm_rectify.h, for the same reason.
 * Scanline optimisation of the right view as a stage, and the test tap on the scanline passes' path-cost sums: declared in
 * stm_hslo_tap.h, for the same reason.
 * Packed 2D-plus-depth video frames as a stream's input (the image and its depth picture in one BGR or NV12 frame, under
 * stm_set_packing's settings): its one entry point is declared, with the definition line by line, in stm_depth_video.h, for the
 * same reason. */
void  stm_stream_destroy(void *stream);

/* ----------------------------------------------------------------- BMP I/O */
/* image_io.cpp:95-112 reads the pair with cv::imread; these read/write the same 24-bit BMPs.
 * stm_bmp_read returns a malloc'd BGR buffer (free with stm_bmp_free) or NULL. */
unsigned char *stm_bmp_read(const char *path, int *num_rows, int *num_cols);
int            stm_bmp_write(const char *path, const unsigned char *bgr, int num_rows, int num_cols);
void           stm_bmp_free(unsigned char *p);

#if defined(STM_BUILD) && defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* STM_HIP_H */
