// stm_views.h -- which camera position an output sub-pixel shows: the device functions the renderer kernels
// (stm_kernels_dibr.hip) and the overlay compositor (stm_kernels_overlay.hip) share, so that neither restates the other's.
// Include from a file compiled -ffp-contract=off (csrc/Makefile): the f64 lines below are one operation each.
#pragma once
#include "stm_common.h"

namespace stm {

// ------------------------------------------------------------------ the reference's view assignment (mux_multiview_kernel_2)
struct MuxGeom { // the reference's view assignment (LMODE 0): mux_multiview_kernel_2's arguments
    float inv_y;
    int ymod;
};
// the view of the R sub-pixel of output pixel (tx, ty); G shows r_view + 1 and B r_view + 2, both modulo N
// (d_mux_multiview.cu:60-73; variant 2 multiplies by 1 / y_interval :62-63, variant 1 divides :105-106)
__device__ __forceinline__ int mux_r_view(int tx, int ty, int N, float y_interval, float inv_y, int ymod, int variant)
{
    const float x_interval = (float)N;
    float y_view = (float)(ty % ymod) + 1.0f;
    y_view = y_view * x_interval;
    y_view = (variant == 2) ? y_view * inv_y : y_view / y_interval;
    int r_view = (tx * 3 + (int)y_view) % N;
    if (r_view < 0) r_view += N;
    return r_view;
}
// the shift view v of N is rendered at: 1 for view 0 (the right image), 0 for view N - 1 (the left image)
__device__ __forceinline__ float view_shift(int v, int N)
{
    return (float)(1.0 - ((1.0 * (double)(float)v) / ((double)(float)N - 1.0))); // d_io.cu:189
}

// ------------------------------------------------------------------ calibrated lenticular interlacing (stm_hip.h, stm_set_lens)
// mux_multiview_kernel_2 takes a sub-pixel's view from (3 tx + int((ty % round(yi) + 1) N / yi)) % N: a lens pitch of exactly N
// sub-pixels, no phase offset, a slant whose row period is rounded to an integer.  Here the view follows from the panel's
// calibration: the lens phase of sub-pixel k = 2 - c of output pixel (tx, ty), in double, one operation per line (the file is
// compiled -ffp-contract=off and the f64 division is the correctly rounded one).  The sampling position (xs, ys) and the
// 4-neighbour sampler stay the reference's.
__device__ __forceinline__ double lens_phase(int tx, int ty, int c, const Lens &g)
{
    const int s = 3 * tx + (2 - c);
    const double t1 = (double)ty * g.slope;
    const double t2 = (double)s + t1;
    const double t3 = t2 / g.pitch;
    const double t4 = t3 + g.centre;
    const double a = t4 - floor(t4);
    return a < 1.0 ? a : 0.0; // a >= 1: t4 was a tiny negative number and the subtraction rounded to 1 (a t4 that is not finite lands here too)
}
// what a phase selects -- MODE 1: the nearest view v; MODE 2: the views v, v + 1 and the weight w of the second; MODE 3: the shift
// of the sub-pixel's own position between the cameras
template <int MODE>
__device__ __forceinline__ void lens_pick(double a, int N, int &v, float &w, float &shift)
{
    double g = a * (double)N;
    v = 0; w = 0.0f; shift = 0.0f;
    if constexpr (MODE == 1) {
        v = min((int)g, N - 1);
    } else {
        g = g - 0.5;
        g = fmin(fmax(g, 0.0), (double)(N - 1)); // the half-bin at either lens edge shows the end view
        if constexpr (MODE == 2) {
            v = min((int)g, N - 2);
            w = (float)(g - (double)v);
        } else {
            const double u = g / (double)(N - 1);
            shift = (float)(1.0 - u);
        }
    }
}

// ------------------------------------------------------------------ quilt output (stm_hip.h, stm_set_layout)
struct QuiltGeom {
    int N, tiles_x, tiles_y, order, tw, th, Hin, Win, Hout, Wout, elem_sz;
    int narrow; // 255 Win Hin + Win Hin / 2 fits 32 bits
};
// where tile k lies: its left column and top row
__device__ __forceinline__ void quilt_tile_origin(const QuiltGeom &g, int k, int &left, int &top)
{
    const int i = k % g.tiles_x, j = k / g.tiles_x;
    left = i * g.tw;
    top = (g.order & 1) ? g.Hout - (j + 1) * g.th : j * g.th;
}

} // namespace stm
