/*
 * stm_depth_input.h -- image-plus-depth input of a frame stream (libstm_hip.so): the one entry point that is not in stm_hip.h.
 * Include it next to stm_hip.h, whose stream calls (stm_stream_create, _submit, _collect ...) it goes with.
 */
#ifndef STM_DEPTH_INPUT_H
#define STM_DEPTH_INPUT_H

#include "stm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(STM_BUILD) && defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* image-plus-depth input: the stream's frames are one image and its depth plane, and the second eye is built on the GPU.  An
 * addition: the reference renders from a stereo pair and its own matcher only.  The plane may be stm_stream_maps' own, a depth
 * camera's, a monocular-depth network's or a 2D-plus-depth video's.
 *   format -1 = off, the default: exactly the stream without this call;  0 = float32;  2 = u8;  3 = u16 little-endian codes
 *             (stm_stream_maps' numbering; 1 is refused).
 *   lo, hi    formats 2 and 3: the map values that code 0 and code maxcode stand for (either polarity); format 0: the limits the
 *             plane's values are clamped to.
 *   fill      0 = constant extension of the background into the holes, 1 = continue the background (mirror);  gate: fill 1 only.
 * A frame (what stm_stream_submit reads and stm_stream_input_buffer hands out) is the image, num_rows * num_cols_sbs * elem_sz
 * bytes, followed at byte P = that size rounded up to a multiple of 16 by the tight plane of num_rows x num_cols codes:
 * P + num_rows * num_cols * {4, 1, 2} bytes.  Of the image the first W = num_cols pixels of a row (pitch num_cols_sbs pixels) and the
 * first three bytes of a pixel are read.  The image is the LEFT eye; disparities are delta = x_right - x_left, smaller is nearer.
 * Definition, f32, one operation per line, no fused multiply-add; per row y:
 *   A. decode, giving disp_l[y][x] = d.
 *      formats 2 and 3, maxcode = 255 or 65535:
 *        q = (float)(((double)hi - (double)lo) / (double)maxcode)     on the host, once
 *        t = (float)code * q
 *        d = lo + t                 (inverts stm_stream_maps' plane: quantising d again by that definition returns the code)
 *      format 0, plane value v:
 *        dmin = fminf(lo, hi);  dmax = fmaxf(lo, hi)
 *        t = fminf(v, dmax)         (a NaN becomes dmax, the far limit)
 *        d = fmaxf(t, dmin)
 *   B. landing:  c(x) = min(max(x + (int)d, 0), W - 1), (int) truncating: stm_dibr_occl's landing rule, so the renderer's own hit
 *      map of the right eye is 0 exactly on the pixels step E fills.
 *   C. winner:  of all x with c(x) = c the smallest d wins, among equal d (-0 = +0) the largest x (the forward warps' tie rule); a
 *      serial ascending loop with d <= d_current produces this.  Order-independent, so the GPU result is deterministic.
 *   D. hit pixels:  disp_r[c] = d(winner), img_r[c][0..2] = img[winner][0..2].
 *   E. holes:  a hole run [a, b] is a maximal run of columns no source reached.
 *        L = a - 1 if a > 0;  R = b + 1 if b < W - 1: both are hit pixels and at least one exists.
 *        the background side B is the only one that exists; with both, L if disp_r[L] > disp_r[R], else R (the farther side; a tie
 *        goes to R).
 *        for every k of the run: disp_r[k] = disp_r[B], and
 *          fill 0:  img_r[k] = img_r[B]
 *          fill 1:  m = 2 B - k;  if 0 <= m < W, m is a hit pixel and fabsf(disp_r[m] - disp_r[B]) <= gate (one f32 subtraction):
 *                   img_r[k] = img_r[m];  otherwise img_r[k] = img_r[B].
 *   F. the frame:  the cut detector and the active-area detector (stm_stream_set_cut, stm_stream_set_active) run on the given image
 *      as the left eye, ahead of steps A to E; the active fill runs on the two maps where the stream's setting asks for it; then the
 *      renderer, the overlay and its placement run on (img, img_r, disp_l, disp_r) exactly as they do behind the matcher.  Where
 *      num_cols_sbs > num_cols the renderer reads a tight copy of the image.  Bytes past a pixel's third are written 0 in img_r and
 *      in that copy.  stages is 3 or 3 | 0x800.
 * One kernel launch per frame (a workgroup per row, the row's winners in LDS: num_cols <= 8192), inside the slot's captured graph.
 * stm_stream_collect and its variants hand out disp_l (the decoded plane), disp_r (the synthesised map) and the frame;
 * stm_stream_maps' formats, the lens, the depth budget, quilts, NV12 output, the overlay, antialiasing, the cut detector and the
 * active area combine with it as with a stereo stream.  Each slot's pinned and device input buffers are allocated anew: pointers
 * handed out by stm_stream_input_buffer before the call are void.
 * Errors (stm_last_error names stream_input_depth; -1, the stream unchanged): a format outside {-1, 0, 2, 3}; lo or hi not finite
 * or beyond +-4096; |hi - lo| < 1/64; a fill outside 0 .. 1; with fill 1 a gate that is not finite or outside [0, 4096]; num_cols >
 * 8192; a call after the first submit; a stream that has NV12 input, a packing, a match size, an alignment or a balance mode other
 * than 0, or stages other than 3 / 3 | 0x800.  In the other direction stm_stream_set_input, _set_packing, _set_match_size,
 * _set_align, _set_balance, and _set_stages for anything but 3 / 3 | 0x800, refuse while depth input is on.  Returns 0.
 * There is no stage call and no frame entry for this input: the stream is its only door.  The entry is
 * declared here and not in stm_hip.h because that header's set of names is recorded in the test suite's screening tables.
 * Where the image and its depth arrive as ONE video frame -- a 2D-plus-depth stream out of a decoder, BGR or NV12, side by side or top
 * and bottom, full or squeezed -- stm_depth_video.h has the entry that reads that frame directly (stm_stream_input_packed_depth). */
int   stm_stream_input_depth(void *stream, int format, float lo, float hi, int fill, float gate);

#if defined(STM_BUILD) && defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* STM_DEPTH_INPUT_H */
