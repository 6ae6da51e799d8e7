/*
 * stm_hslo_tap.h -- scanline optimisation (stm_dc_hslo / stm_d_dc_hslo, stages bit 0x100 of the frame calls; libstm_hip.so): the
 * right view as a stage, and test access to the path-cost sums of the four passes.  Include it next to stm_hip.h, whose conventions
 * (device flavour, stm_last_error, the error modes) it goes with.
 */
#ifndef STM_HSLO_TAP_H
#define STM_HSLO_TAP_H

#include "stm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(STM_BUILD) && defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Test access to the scanline passes of the calling thread: where the four directions' path costs are summed, a copy leaves.
 * Each argument is null or a device buffer of [views][D][H][W] float32, 4-byte aligned, fully sized by the caller, image columns
 * only (no padding of the library's own layouts): views = 1 for stm_dc_hslo, stm_d_dc_hslo and stm_d_dc_hslo_view, 2 (left view,
 * then right view) for a frame call with stages bit 0x100; D, H, W = the num_disp, num_rows, num_cols of that call.
 *   d_s2   the accumulator behind the two horizontal passes:  C_lr + C_rl
 *   d_s3   the accumulator behind the top-to-bottom pass:     (C_lr + C_rl) + C_tb
 *   d_fin  the final volume, which the library never stores:  (((C_lr + C_rl) + C_tb) + C_bt) * 0.25f -- the winner-takes-all map
 *          of the call is the first lowest hypothesis of this volume
 * d_s2 and d_s3 are copy kernels of their own behind the passes; d_fin is written by the bottom-to-top kernel itself, the same
 * kernel that runs with the tap clear (a wave tests the pointer once, ahead of its walk over the rows, and walks them with or
 * without the store; both walks are compiled from the same lines).  All three null = off, the default: no launch is added
 * and no result changes.  Every scanline run the thread enqueues while the tap is set fills the buffers that are set; the caller
 * keeps them alive until those runs have finished.  A frame stream refuses stages bit 0x100, so a stream never runs the tap.
 * Returns 0, or -1 with stm_last_error set (it names set_hslo_tap) and the tap unchanged for a pointer that is not 4-byte aligned
 * (an error like any other: the default error mode exits). */
int   stm_set_hslo_tap(float *d_s2, float *d_s3, float *d_fin);

/* stm_d_dc_hslo for either view of a pair.  d_cost is the view's own aggregated volume (a device table of num_disp plane
 * pointers), d_img_own the view's own image and d_img_other the other one, both num_rows x num_cols x elem_sz in device memory.
 * view 0 = the left view: the matched pixel of x at hypothesis d is x + (d - zero_disp); exactly stm_d_dc_hslo(d_cost, d_disp,
 * d_img_own, d_img_other, ...).  view 1 = the right view: the matched pixel is x - (d - zero_disp), which is what a frame call with
 * stages bit 0x100 runs for its right map with the right image as d_img_own and the left one as d_img_other.
 * Asynchronous on stm_set_stream's stream.  Refused before anything is launched (stm_last_error names d_dc_hslo_view): num_disp,
 * num_rows or num_cols < 1, elem_sz < 3, a view other than 0 or 1. */
void  stm_d_dc_hslo_view(float **d_cost, float *d_disp, unsigned char *d_img_own, unsigned char *d_img_other,
                         float T, float H1, float H2, int num_disp, int zero_disp,
                         int num_rows, int num_cols, int elem_sz, int view);

#if defined(STM_BUILD) && defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* STM_HSLO_TAP_H */
