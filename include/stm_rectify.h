/*
 * stm_rectify.h -- rectification from camera calibration (libstm_hip.so): both eyes of a calibrated two-camera rig remapped on the
 * GPU, as a stage and as the first step of a frame stream's frames.  Include it next to stm_hip.h, whose conventions (host and
 * device flavours, stm_last_error, the stream calls) it goes with.
 */
#ifndef STM_RECTIFY_H
#define STM_RECTIFY_H

#include "stm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(STM_BUILD) && defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* rectification: an addition, the reference takes rectified studio masters.  Everything behind it (the matcher, the cross arms, the
 * L/R check, every warp of the renderer) assumes that a scene point lies on the same row in both eyes; this step makes it so from
 * what a calibration delivers: a camera matrix, distortion coefficients and a rectifying rotation per camera.
 * One eye has one record of 18 floats c[0..17]:
 *   c[0..8]    m00 m01 m02 m10 m11 m12 m20 m21 m22: rectified pixel to camera ray, the inverse of newK * R in OpenCV's terms
 *   c[9..12]   fx fy cx cy: the camera matrix of the unrectified image
 *   c[13..17]  k1 k2 p1 p2 k3: Brown-Conrady distortion coefficients
 * Definition, for output pixel (x, y) of an H x W eye, xf = (float)x, yf = (float)y; f32, one operation per line, no fused
 * multiply-add, the division correctly rounded:
 *   A. the ray:
 *        X = m00*xf;  t = m01*yf;  X = X + t;  X = X + m02          (Y with m10 m11 m12, Wd with m20 m21 m22 likewise)
 *        xn = X / Wd;  yn = Y / Wd
 *   B. the distortion:
 *        xx = xn*xn;  yy = yn*yn;  xy = xn*yn;  r2 = xx + yy
 *        rad = k3*r2;  rad = rad + k2;  rad = rad*r2;  rad = rad + k1;  rad = rad*r2;  rad = rad + 1
 *        a = xy + xy;  a = p1*a;  b = xx + xx;  b = r2 + b;  b = p2*b;  xd = xn*rad;  xd = xd + a;  xd = xd + b
 *        a = yy + yy;  a = r2 + a;  a = p1*a;  b = xy + xy;  b = p2*b;  yd = yn*rad;  yd = yd + a;  yd = yd + b
 *   C. the source position, in 1/32 pixel:
 *        u = fx*xd;  u = u + cx;      v = fy*yd;  v = v + cy
 *        mu = u*32;  mu = mu + 0.5;  mu = floorf(mu)                 (mv from v likewise)
 *        ok = mu >= -1048576 && mu <= 1048576 && mv >= -1048576 && mv <= 1048576      (a NaN fails it)
 *      !ok: the pixel is 0 in all three channels, with either border.
 *      otherwise qu = (int)mu, x0 = qu >> 5 (arithmetic shift), fu = qu & 31; y0 and fv from mv likewise.
 *   D. the taps:  (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), values p00 p01 p10 p11.
 *        border 0: a tap outside [0, W) x [0, H) is 0;   border 1: its coordinates are clamped to the eye.
 *   E. the blend, per channel, in exact integers:
 *        top = (32-fu)*p00 + fu*p01;  bot = (32-fu)*p10 + fu*p11;  out = ((32-fv)*top + fv*bot + 512) >> 10
 * The identity record (m = I, fx = fy = 1, everything else 0) is a copy.
 * The source is the unpacked, converted BGR eye: with NV12 input or a packing (stm_stream_set_input, stm_stream_set_packing) a tap
 * is the pixel the unpacking and the conversion give, fetched on the fly.  DESIGN.md section 32. */

/* One image through one record: img_out (num_rows x num_cols x elem_sz) from img.  Host flavour (stm_rectify: both images in host
 * memory, bytes of a pixel past the third come back 0) and device flavour (stm_d_rectify: both in device memory at any byte address,
 * bytes past the third left to the caller; asynchronous on stm_set_stream's stream) as stm_align_rows / stm_d_align_rows.  rec18 is
 * a host pointer in both.  Refused before anything is launched or written (stm_last_error names rectify / d_rectify): a null
 * pointer; num_rows or num_cols outside 1 .. 16384; elem_sz < 3; a border other than 0 or 1; a record with a float that is not
 * finite; img_out overlapping img. */
void  stm_rectify(unsigned char *img_out, const unsigned char *img, const float *rec18, int num_rows, int num_cols, int elem_sz, int border);
void  stm_d_rectify(unsigned char *d_img_out, const unsigned char *d_img, const float *rec18, int num_rows, int num_cols, int elem_sz, int border);
/* A test tap on steps A to C, host flavour only: quv receives num_rows x num_cols x 2 int32 (qu, qv), both INT32_MIN where !ok.
 * Refusals as above, where they apply. */
void  stm_rectify_coords(int *quv, const float *rec18, int num_rows, int num_cols);

/* The rectification of a frame stream.  mode 0 = off, the default: exactly the stream without this call (rec36 may be null);
 * mode 1: rec36 is the left eye's record followed by the right eye's.  The records are copied into the stream and handed to the
 * kernel by value: no device allocation, nothing that changes between the frames of a captured graph.
 * The step is the first thing a frame does, ahead of the cut detector, the active area, the alignment and the balance: one launch
 * writes both rectified eyes as one side-by-side BGR frame, and from there the frame is, by definition, the stream's frame on the
 * rectified pair (plain BGR, num_cols_sbs = 2 * num_cols, no packing, no NV12 planes) -- every later setting, stages bit, match size
 * and captured graph as it is.  With stages bit 0x2000 the previous frame goes through the same kernel with the same records.
 * Errors (stm_last_error names stream_rectify; -1, the stream unchanged): a mode other than 0 or 1; in mode 1 a null rec36, a float
 * that is not finite or a border other than 0 or 1; a BGR stream without a packing whose num_cols_sbs < 2 * num_cols; a stream
 * with depth input (stm_stream_input_depth, which in turn refuses while a rectification is on: an image-plus-depth frame is not
 * rectified); a call after the first submit.  Returns 0.
 * There is no thread-level setter for the frame entries: the stream is the only door. */
int   stm_stream_rectify(void *stream, int mode, const float *rec36, int border);
/* reads the setting back: *mode, and with a rectification on the 36 floats and *border (each pointer may be null) */
int   stm_stream_get_rectify(void *stream, int *mode, float *rec36, int *border);

#if defined(STM_BUILD) && defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* STM_RECTIFY_H */
