/*
 * stm_depth_video.h -- packed 2D-plus-depth video frames as the input of a frame stream (libstm_hip.so): the image and its depth
 * picture in one BGR or NV12 frame.  One entry point, next to stm_depth_input.h's; include it with stm_hip.h, whose stream calls
 * (stm_stream_create, _submit, _collect ...) it goes with.
 */
#ifndef STM_DEPTH_VIDEO_H
#define STM_DEPTH_VIDEO_H

#include "stm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(STM_BUILD) && defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* packed 2D-plus-depth input: the stream's frames are single video frames that hold the image in one half and its depth, as a grey
 * picture, in the other half -- side by side or top and bottom, full size or squeezed to half the columns or rows: the "2D+Z"
 * family, the depth tracks of depth-video encoders, stm_stream_maps' own plane once it went through an encoder.  The frame is read
 * as a decoder leaves it; nothing is converted, cut out or resampled on the CPU.  An addition: the reference renders from a stereo
 * pair and its own matcher only.
 *   format  -1 = off, the default: exactly the stream without this call;  0 = BGR frame;  1 = NV12 frame.
 *   matrix  stm_demux_nv12's, 0 .. 3; ignored for format 0.
 *   packing, swap, filter, gap   stm_demux_packed's settings and geometry table.  Eye 0 is the image (the LEFT eye), eye 1 the depth
 *           picture; swap 1: the depth picture comes first.  num_rows x num_cols is the size of the unpacked image.  filter applies
 *           to the image only.  In NV12 mode the evenness rules of stm_demux_nv12_packed apply.
 *   range, dfilter, dgate, lo, hi   how the depth picture is decoded, steps A' to A'''.
 *   fill, gate   stm_stream_input_depth's (step E of stm_depth_input.h).
 * A frame (what stm_stream_submit reads and stm_stream_input_buffer hands out) is rows_f * num_cols_sbs * elem_sz bytes; in NV12
 * mode rows_f * num_cols_sbs * 3 / 2 bytes, the UV plane at byte rows_f * num_cols_sbs and both pitches num_cols_sbs: exactly
 * stm_stream_set_packing's rules.  Disparities are delta = x_right - x_left, smaller is nearer.
 * Definition; per pixel (x, y) of the image, 0 <= x < num_cols, 0 <= y < num_rows:
 *   0.    the image:  img[y][x] is, by definition, pixel (x, y) of eye 0 of stm_demux_packed (format 0) or stm_demux_nv12_packed
 *         (format 1) on the frame.  The renderer reads a tight BGR copy of it; bytes past a pixel's third are written 0.
 *   A'.   the depth sample at frame pixel (row, col) of the depth picture's region:
 *           format 1: sample = the Y byte at (row, col); the chroma of the depth picture is not read
 *           format 0: sample = byte 1 (G) of the pixel at (row, col)
 *           range 0:  c = sample;                            M = 255
 *           range 1:  c = min(max(sample, 16), 235) - 16;    M = 219     (limited-range video grey)
 *   A''.  expansion, in quarter codes; all arithmetic is 32-bit integer.  P[i] is the depth picture's sample i along the packing
 *         axis at this pixel's other coordinate; a = x (packings 0, 1) or y (packings 2, 3):
 *           packings 0 and 2 (dfilter must be 0):  v = 4 c(P[a])
 *           packings 1 and 3:  k = a >> 1;  s = +1 if a is odd else -1;  n = clamp(k + s, 0, last), last = the depth picture's last
 *                              sample along the axis (never the gap or the image)
 *             c0 = c(P[k]);  c1 = c(P[n])
 *             dfilter 0:  v = 4 c0                                     (the sample is replicated: no depth is invented across an edge)
 *             dfilter 1:  v = |c0 - c1| <= dgate ? 3 c0 + c1 : 4 c0    (the packing's linear position k -+ 1/4, only inside a surface)
 *   A'''. decode, f32, one operation per line, no fused multiply-add:
 *           q4 = (float)(((double)hi - (double)lo) / (4.0 * M))     on the host, once
 *           t = (float)v * q4
 *           d = lo + t                  giving disp_l[y][x] = d.  lo and hi may have either polarity.  With range 0 and v = 4 c this
 *                                       is stm_stream_input_depth's format-2 decode of code c bit for bit: scaling by 4 is exact in f32.
 *   B to F.  stm_depth_input.h's steps B to F, verbatim, on this image and this disp_l; fill and gate as there.  The cut detector
 *         and the active-area detector read the image half of the frame as the left eye; the depth half never reaches them.
 *         stages is 3 or 3 | 0x800.
 * One kernel launch per frame (a workgroup per row, the row's winners in LDS: num_cols <= 8192), inside the
 * slot's captured graph.  stm_stream_collect and its variants hand out disp_l (the decoded depth picture), disp_r (the synthesised
 * map) and the frame; the settings that stm_depth_input.h lists combine with it in the same way.  Each slot's pinned and device
 * input buffers are allocated anew: pointers handed out by stm_stream_input_buffer before the call are void.
 * Errors (stm_last_error names stream_input_packed_depth; -1, the stream unchanged): a format outside {-1, 0, 1}; what
 * stm_demux_packed (format 0) or stm_demux_nv12_packed (format 1) refuse of packing, swap, filter, gap, matrix and the stream's
 * num_rows, num_cols_sbs, num_cols; in NV12 mode an odd num_cols_sbs; a range or a dfilter outside 0 .. 1; dfilter 1 with packing 0
 * or 2; a dgate outside 0 .. 255; what stm_stream_input_depth refuses of lo, hi, fill and gate; num_cols > 8192; a call after the
 * first submit; a stream that has stm_stream_input_depth on, NV12 input (stm_stream_set_input) or a packing
 * (stm_stream_set_packing), a match size, an alignment, a balance or a rectification mode other than 0, or stages other than 3 /
 * 3 | 0x800.  In the other direction stm_stream_input_depth, stm_stream_set_input, _set_packing, _set_match_size, _set_align,
 * _set_balance, stm_stream_rectify, and _set_stages for anything but 3 / 3 | 0x800, refuse while this input is on.  Returns 0.
 * Not covered: the image as the right eye, depth coded in more than 8 bits or in chroma, P010, the header pixels of the Dimenco
 * format.  There is no stage call and no frame entry for this input: the stream is its only door. */
int   stm_stream_input_packed_depth(void *stream, int format, int matrix, int packing, int swap, int filter, int gap, int range,
                                    int dfilter, int dgate, float lo, float hi, int fill, float gate);

#if defined(STM_BUILD) && defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* STM_DEPTH_VIDEO_H */
