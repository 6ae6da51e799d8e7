// stm_kernels_overlay.hip -- an overlay (subtitles, a logo, a player's OSD) composited into a finished frame at a chosen depth,
// for gfx950 (include/stm_hip.h, stm_mux_overlay).
//
// The frame is finished: interlaced (the reference's view assignment or a lens geometry) or a quilt.  Every sub-pixel of it shows
// one camera position s in [0, 1]; the overlay appears there shifted by (s - 0.5) * disparity view pixels, so the eye fuses it at
// that disparity.  One kernel over the overlay's bounding box does it for every output form, with the renderer's own device
// functions for s (stm_views.h): a fused option in each renderer kernel would multiply their forms again.
//
// A thread owns RUN consecutive output pixels of one row.  Where the run lies inside the box and its first byte is dword aligned
// (always, for a 4-byte aligned frame whose row is a multiple of 4 bytes) the run is read as dwords and, with 3-byte pixels,
// written as dwords; 4-byte pixels are written as a 16-bit and an 8-bit store, which leaves the fourth byte alone.  Everything
// else takes the byte path.  An overlay pixel is one aligned dword load; the sub-pixels of a row's neighbouring pixels read the
// same cache lines.  No LDS, no scratch.
#include "stm_common.h"
#include "stm_views.h"

#pragma clang fp contract(off) // the position's f64 lines are one operation each (the Makefile's -ffp-contract=off says the same)

namespace stm {

namespace {
constexpr int OV_RUN = 4;                 // output pixels per thread
constexpr int OV_BX = 64, OV_BY = 4;      // a block: 64 runs of 4 rows (four waves, one row each)
enum { OV_MUX = 0, OV_LENS_VIEW = 1, OV_LENS_SHIFT = 3, OV_QUILT = 4 };
} // namespace

struct OverlayArgs {
    u8 *out;              // the frame, Wout pixels a row
    const uint32_t *ov;   // ov_rows x ov_cols pixels B, G, R, A, premultiplied
    int ov_rows, ov_cols, x0, y0;
    float disparity;
    const float *d_disp;       // the disparity read on the device instead, clamped to [limit_lo, limit_hi] (stm_set_overlay_auto); null = `disparity`
    float limit_lo, limit_hi;
    int N, Wout, elem_sz;
    int bx0, bx1, by0, by1; // the bounding box in view pixel space (non-empty)
    float y_interval;       // OV_MUX
    MuxGeom mg;             // OV_MUX
    Lens g;                 // OV_LENS_*
    QuiltGeom q;            // OV_QUILT
};

// where view pixel column x samples overlay row `row` under shift s, and the two interpolated words (stm_hip.h, steps 2 and 3):
// I_c for the colour byte c and I_3 for alpha
struct OvTap {
    uint32_t p0, p1, fr;
};
__device__ __forceinline__ OvTap overlay_tap(const OverlayArgs &a, float disparity, const uint32_t *__restrict__ row, int x, float s)
{
    const double t = (double)s - 0.5;
    const double o = (double)disparity * t;
    double p = (double)((long long)x - (long long)a.x0) - o;
    p = p * 256.0;
    const long long F = (long long)floor(p);
    const long long q = F >> 8;
    OvTap r;
    r.fr = (uint32_t)(F & 255);
    r.p0 = (q >= 0 && q < a.ov_cols) ? row[q] : 0u;
    r.p1 = (q + 1 >= 0 && q + 1 < a.ov_cols) ? row[q + 1] : 0u;
    return r;
}
__device__ __forceinline__ uint32_t overlay_blend(const OvTap &t, int c, uint32_t dst)
{
    const uint32_t ic = (256u - t.fr) * ((t.p0 >> (8 * c)) & 255u) + t.fr * ((t.p1 >> (8 * c)) & 255u);
    const uint32_t ia = (256u - t.fr) * (t.p0 >> 24) + t.fr * (t.p1 >> 24);
    const uint32_t v = (255u * ic + (65280u - ia) * dst + 32640u) / 65280u;
    return min(v, 255u);
}
// the three bytes of view pixel (x, y) -- output pixel (ox, oy) -- composited: px = B | G << 8 | R << 16 in, the same out
template <int MODE>
__device__ __forceinline__ uint32_t overlay_pixel(const OverlayArgs &a, float disparity, const uint32_t *__restrict__ row, int x, int ox, int oy,
                                                  float s_tile, uint32_t px)
{
    uint32_t r = 0;
    if constexpr (MODE == OV_QUILT) { // one view per tile: the three bytes share the tap
        const OvTap t = overlay_tap(a, disparity, row, x, s_tile);
#pragma unroll
        for (int c = 0; c < 3; ++c) r |= overlay_blend(t, c, (px >> (8 * c)) & 255u) << (8 * c);
    } else {
        int r_view = 0;
        if constexpr (MODE == OV_MUX) r_view = mux_r_view(ox, oy, a.N, a.y_interval, a.mg.inv_y, a.mg.ymod, 2);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float s;
            if constexpr (MODE == OV_MUX) {
                int v = r_view + (2 - c); // byte 0 = the b view (r + 2), byte 2 = the r view
                if (v >= a.N) v -= a.N;
                s = view_shift(v, a.N);
            } else {
                int v;
                float w, shift;
                lens_pick<MODE>(lens_phase(ox, oy, c, a.g), a.N, v, w, shift);
                s = MODE == OV_LENS_VIEW ? view_shift(v, a.N) : shift;
            }
            const OvTap t = overlay_tap(a, disparity, row, x, s);
            r |= overlay_blend(t, c, (px >> (8 * c)) & 255u) << (8 * c);
        }
    }
    return r;
}

template <int MODE>
__global__ __launch_bounds__(OV_BX * OV_BY) void stm_k_overlay(OverlayArgs a)
{
    const int y = a.by0 + (int)blockIdx.y * OV_BY + (int)threadIdx.y; // view row
    if (y >= a.by1) return;
    int left = 0, top = 0;
    float s_tile = 0.0f;
    if constexpr (MODE == OV_QUILT) {
        const int k = (int)blockIdx.z;
        quilt_tile_origin(a.q, k, left, top);
        s_tile = view_shift((a.q.order & 2) ? a.N - 1 - k : k, a.N);
    }
    // runs are aligned on the output column, so a row's runs start on multiples of OV_RUN pixels
    const int lo = left + a.bx0, hi = left + a.bx1, oy = top + y;
    const int ox0 = (lo & ~(OV_RUN - 1)) + ((int)blockIdx.x * OV_BX + (int)threadIdx.x) * OV_RUN;
    if (ox0 >= hi) return;
    const uint32_t *__restrict__ row = a.ov + (size_t)(y - a.y0) * a.ov_cols;
    // one pointer test: the fitted disparity of this frame, written earlier on the same stream (C fmaxf: a NaN becomes limit_lo)
    const float disparity = a.d_disp ? fminf(fmaxf(*a.d_disp, a.limit_lo), a.limit_hi) : a.disparity;
    u8 *p = a.out + ((size_t)oy * a.Wout + ox0) * a.elem_sz;
    const bool whole = ox0 >= lo && ox0 + OV_RUN <= hi && ((uintptr_t)p & 3) == 0;
    if (whole && a.elem_sz == 3) {
        uint32_t *d = (uint32_t *)p;
        const uint32_t w0 = d[0], w1 = d[1], w2 = d[2];
        const uint32_t r0 = overlay_pixel<MODE>(a, disparity, row, ox0 - left, ox0, oy, s_tile, w0 & 0xffffffu);
        const uint32_t r1 = overlay_pixel<MODE>(a, disparity, row, ox0 + 1 - left, ox0 + 1, oy, s_tile, (w0 >> 24) | ((w1 & 0xffffu) << 8));
        const uint32_t r2 = overlay_pixel<MODE>(a, disparity, row, ox0 + 2 - left, ox0 + 2, oy, s_tile, (w1 >> 16) | ((w2 & 0xffu) << 16));
        const uint32_t r3 = overlay_pixel<MODE>(a, disparity, row, ox0 + 3 - left, ox0 + 3, oy, s_tile, w2 >> 8);
        d[0] = r0 | (r1 << 24);
        d[1] = (r1 >> 8) | (r2 << 16);
        d[2] = (r2 >> 16) | (r3 << 8);
        return;
    }
    if (whole && a.elem_sz == 4) {
        const uint32_t *d = (const uint32_t *)p;
        uint32_t w[OV_RUN];
#pragma unroll
        for (int i = 0; i < OV_RUN; ++i) w[i] = d[i];
#pragma unroll
        for (int i = 0; i < OV_RUN; ++i) {
            const uint32_t r = overlay_pixel<MODE>(a, disparity, row, ox0 + i - left, ox0 + i, oy, s_tile, w[i] & 0xffffffu);
            *(uint16_t *)(p + 4 * i) = (uint16_t)r; // the fourth byte is never written
            p[4 * i + 2] = (u8)(r >> 16);
        }
        return;
    }
    for (int i = 0; i < OV_RUN; ++i) { // the box's edges, unaligned frames, wider pixels
        const int ox = ox0 + i;
        if (ox < lo || ox >= hi) continue;
        u8 *o = p + (size_t)i * a.elem_sz;
        const uint32_t px = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16);
        const uint32_t r = overlay_pixel<MODE>(a, disparity, row, ox - left, ox, oy, s_tile, px);
        o[0] = (u8)r; o[1] = (u8)(r >> 8); o[2] = (u8)(r >> 16);
    }
}

// The overlay `ov` composited in place on the finished frame `out` (Hout x Wout x elem_sz).  lo.layout 0: interlaced under ln
// (ln.mode 0: the reference's view assignment from y_interval, inv_y_interval and ymod); 1: a quilt, screened by quilt_args_ok.
// The arguments have been screened by the caller (stm_api.hip, overlay_args_ok); an empty bounding box launches nothing.
void launch_overlay(u8 *out, const u8 *ov, int ov_rows, int ov_cols, int x0, int y0, float disparity, int N, const Lens &ln,
                    float y_interval, float inv_y_interval, int ymod, const Layout &lo, int Hout, int Wout, int elem_sz, const float *d_disp,
                    float limit_lo, float limit_hi)
{
    OverlayArgs a = {};
    a.out = out; a.ov = (const uint32_t *)ov;
    a.ov_rows = ov_rows; a.ov_cols = ov_cols; a.x0 = x0; a.y0 = y0; a.disparity = disparity;
    a.d_disp = d_disp; a.limit_lo = limit_lo; a.limit_hi = limit_hi;
    a.N = N; a.Wout = Wout; a.elem_sz = elem_sz;
    a.y_interval = y_interval; a.mg = MuxGeom{inv_y_interval, ymod}; a.g = ln;
    int Hv = Hout, Wv = Wout, tiles = 1;
    if (lo.layout == 1) {
        a.q = QuiltGeom{N, lo.tiles_x, lo.tiles_y, lo.order, Wout / lo.tiles_x, Hout / lo.tiles_y, 0, 0, Hout, Wout, elem_sz, 0};
        Hv = a.q.th; Wv = a.q.tw; tiles = N;
    }
    // |x0|, |y0| <= 65536, the overlay's sides <= 65535, |disparity| <= 4096: every sum below stays far inside an int
    // a disparity read on the device is only known by its limits here: the box takes the larger one's margin, and the columns that
    // adds sample (0, 0, 0, 0), which leaves a frame byte exactly as it is
    const int m = (int)ceilf((d_disp ? fmaxf(fabsf(limit_lo), fabsf(limit_hi)) : fabsf(disparity)) * 0.5f) + 1;
    a.by0 = y0 > 0 ? y0 : 0;
    a.by1 = y0 + ov_rows < Hv ? y0 + ov_rows : Hv;
    a.bx0 = x0 - m > 0 ? x0 - m : 0;
    a.bx1 = x0 + ov_cols + m < Wv ? x0 + ov_cols + m : Wv;
    if (a.by0 >= a.by1 || a.bx0 >= a.bx1) return;
    // the widest row of runs over the tiles: a tile's left column shifts the alignment by at most OV_RUN - 1 pixels
    const int runs = cdiv(a.bx1 - a.bx0 + OV_RUN - 1, OV_RUN);
    const dim3 grid(cdiv(runs, OV_BX), cdiv(a.by1 - a.by0, OV_BY), tiles), block(OV_BX, OV_BY);
    ProfScope p("overlay");
    if (lo.layout == 1) STM_LAUNCH(stm_k_overlay<OV_QUILT>, grid, block, 0, stream(), a);
    else if (ln.mode == 0) STM_LAUNCH(stm_k_overlay<OV_MUX>, grid, block, 0, stream(), a);
    else if (ln.mode == 1) STM_LAUNCH(stm_k_overlay<OV_LENS_VIEW>, grid, block, 0, stream(), a);
    else STM_LAUNCH(stm_k_overlay<OV_LENS_SHIFT>, grid, block, 0, stream(), a);
    STM_CHECK_LAUNCH();
}

} // namespace stm
