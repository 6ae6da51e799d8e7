// stm_kernels_rectify.hip -- rectification from camera calibration (stm_rectify, stm_stream_rectify; include/stm_rectify.h has the
// definition line by line).  An addition, the reference has nothing like it: it takes rectified studio masters.  Two kernels:
//   stm_k_rectify         both eyes of a frame call's input (BGR or NV12, any packing, read through stm_fetch.h) remapped through
//                         their records into one side-by-side BGR frame, which the plain frame path then takes; with one image it is
//                         the stage stm_d_rectify.  A lane owns four consecutive pixels of the output: the coordinate chain runs once
//                         per pixel, the four taps come as packed pixels, the blend runs on the packed words (B and R in one word's
//                         16-bit halves for the horizontal step), and the workspace frame leaves as three dwords (3-byte pixels) or
//                         one dwordx4 (4-byte pixels) per lane.  A caller's buffer that is not dword aligned, or whose pixels keep
//                         their bytes past the third, takes byte stores.  No LDS, no scratch.
//   stm_k_rectify_coords  the test tap: the chain's (qu, qv) per pixel.
// The records are kernel arguments (by value): no device memory of their own, nothing that changes between the frames of a graph.
#include "stm_common.h"
#include "stm_fetch.h"

namespace stm {

namespace {

struct RectifyRecs {
    float rec[2][18];
};

// the definition's chain for output pixel (x, y) through record e: f32, one operation per line (the file is compiled
// -ffp-contract=off; the division is the correctly rounded one).  false where the pixel is not ok
__device__ __forceinline__ bool rect_coords(const RectifyRecs &r, int e, int x, int y, int &qu, int &qv)
{
#define RC(i) (e ? r.rec[1][i] : r.rec[0][i])
    const float xf = (float)x, yf = (float)y;
    float X = RC(0) * xf;
    float t = RC(1) * yf;
    X = X + t;
    X = X + RC(2);
    float Y = RC(3) * xf;
    t = RC(4) * yf;
    Y = Y + t;
    Y = Y + RC(5);
    float Wd = RC(6) * xf;
    t = RC(7) * yf;
    Wd = Wd + t;
    Wd = Wd + RC(8);
    const float xn = X / Wd;
    const float yn = Y / Wd;
    const float xx = xn * xn;
    const float yy = yn * yn;
    const float xy = xn * yn;
    const float r2 = xx + yy;
    float rad = RC(17) * r2;
    rad = rad + RC(14);
    rad = rad * r2;
    rad = rad + RC(13);
    rad = rad * r2;
    rad = rad + 1.0f;
    float a = xy + xy;
    a = RC(15) * a;
    float b = xx + xx;
    b = r2 + b;
    b = RC(16) * b;
    float xd = xn * rad;
    xd = xd + a;
    xd = xd + b;
    a = yy + yy;
    a = r2 + a;
    a = RC(15) * a;
    b = xy + xy;
    b = RC(16) * b;
    float yd = yn * rad;
    yd = yd + a;
    yd = yd + b;
    float u = RC(9) * xd;
    u = u + RC(11);
    float v = RC(10) * yd;
    v = v + RC(12);
#undef RC
    float mu = u * 32.0f;
    mu = mu + 0.5f;
    mu = floorf(mu);
    float mv = v * 32.0f;
    mv = mv + 0.5f;
    mv = floorf(mv);
    const bool ok = mu >= -1048576.0f && mu <= 1048576.0f && mv >= -1048576.0f && mv <= 1048576.0f; // (a NaN fails it)
    qu = ok ? (int)mu : 0;
    qv = ok ? (int)mv : 0;
    return ok;
}

// one tap: border 1 clamps its coordinates; border 0 reads the clamped address too (always a valid one) and drops what lay outside
template <int FMT, int AXIS, int FILT>
__device__ __forceinline__ uint32_t rect_tap(const AlignSrc &s, int e, int ty, int tx, int H, int W, int border)
{
    const int cy = min(max(ty, 0), H - 1), cx = min(max(tx, 0), W - 1);
    const uint32_t px = al_unpacked_px<FMT, AXIS, FILT>(s, e, cy, cx);
    return (border || (cy == ty && cx == tx)) ? px : 0u;
}

// the pixel of output column x (0 <= x < out_cols), row y: eye e = x >= W of a frame, the one image otherwise
template <int FMT, int AXIS, int FILT>
__device__ __forceinline__ uint32_t rect_px(const AlignSrc &s, const RectifyRecs &r, int two_eyes, int x, int y, int H, int W, int border)
{
    const int e = (two_eyes && x >= W) ? 1 : 0, ex = x - e * W;
    int qu, qv;
    if (!rect_coords(r, e, ex, y, qu, qv)) return 0u;
    const int x0 = qu >> 5, y0 = qv >> 5;
    const uint32_t fu = (uint32_t)(qu & 31), fv = (uint32_t)(qv & 31), gu = 32u - fu, gv = 32u - fv;
    const uint32_t p00 = rect_tap<FMT, AXIS, FILT>(s, e, y0, x0, H, W, border), p01 = rect_tap<FMT, AXIS, FILT>(s, e, y0, x0 + 1, H, W, border);
    const uint32_t p10 = rect_tap<FMT, AXIS, FILT>(s, e, y0 + 1, x0, H, W, border), p11 = rect_tap<FMT, AXIS, FILT>(s, e, y0 + 1, x0 + 1, H, W, border);
    // horizontally on the packed words: B and R in the two halves of one word (13 bits each), G in a word of its own
    const uint32_t tbr = gu * (p00 & 0xff00ffu) + fu * (p01 & 0xff00ffu), tg = gu * ((p00 >> 8) & 0xffu) + fu * ((p01 >> 8) & 0xffu);
    const uint32_t bbr = gu * (p10 & 0xff00ffu) + fu * (p11 & 0xff00ffu), bg = gu * ((p10 >> 8) & 0xffu) + fu * ((p11 >> 8) & 0xffu);
    // vertically per channel: 18 bits
    const uint32_t ob = (gv * (tbr & 0xffffu) + fv * (bbr & 0xffffu) + 512u) >> 10;
    const uint32_t og = (gv * tg + fv * bg + 512u) >> 10;
    const uint32_t orr = (gv * (tbr >> 16) + fv * (bbr >> 16) + 512u) >> 10;
    return ob | (og << 8) | (orr << 16);
}

// npx = H * out_cols pixels of the output, four per lane.  wide: out is dword aligned (elem_sz 3) or 16-byte aligned (elem_sz 4) and
// whole pixels may be written: packed stores; otherwise three byte stores per pixel
template <int FMT, int AXIS, int FILT>
__global__ __launch_bounds__(256) void stm_k_rectify(u8 *__restrict__ out, AlignSrc s, RectifyRecs r, int H, int W, int two_eyes, int out_cols,
                                                     uint32_t npx, int border, int wide)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= (npx + 3u) / 4u) return;
    const uint32_t p = g * 4u;
    int y = (int)(p / (uint32_t)out_cols), x = (int)(p - (uint32_t)y * (uint32_t)out_cols);
    const uint32_t n = min(4u, npx - p);
    uint32_t px[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        px[i] = 0u;
        if ((uint32_t)i < n) px[i] = rect_px<FMT, AXIS, FILT>(s, r, two_eyes, x, y, H, W, border);
        if (++x == out_cols) { x = 0; ++y; }
    }
    if (wide && n == 4u) {
        if (s.elem_sz == 3) {
            uint32_t *d = (uint32_t *)(out + (size_t)g * 12);
            d[0] = px[0] | (px[1] << 24);
            d[1] = (px[1] >> 8) | (px[2] << 16);
            d[2] = (px[2] >> 16) | (px[3] << 8);
        } else {
            *(uint4 *)(out + (size_t)g * 16) = make_uint4(px[0], px[1], px[2], px[3]);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if ((uint32_t)i < n) {
            u8 *d = out + ((size_t)p + i) * s.elem_sz;
            d[0] = (u8)px[i]; d[1] = (u8)(px[i] >> 8); d[2] = (u8)(px[i] >> 16);
            if (wide && s.elem_sz == 4) d[3] = 0; // (the last lane of a wide frame)
        }
    }
}

__global__ __launch_bounds__(256) void stm_k_rectify_coords(int *__restrict__ quv, RectifyRecs r, int H, int W)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    int qu, qv;
    const bool ok = rect_coords(r, 0, x, y, qu, qv);
    int *d = quv + ((size_t)y * W + x) * 2;
    d[0] = ok ? qu : INT32_MIN;
    d[1] = ok ? qv : INT32_MIN;
}

struct RectifyLaunch {
    u8 *out;
    AlignSrc s;
    RectifyRecs r;
    int H, W, two_eyes, out_cols, border, wide;
    template <int FMT, int AXIS, int FILT> void run() const
    {
        const uint32_t npx = (uint32_t)H * (uint32_t)out_cols, groups = (npx + 3u) / 4u;
        STM_LAUNCH((stm_k_rectify<FMT, AXIS, FILT>), dim3((groups + 255u) / 256u), dim3(256), 0, stream(), out, s, r, H, W, two_eyes, out_cols, npx,
                   border, wide);
    }
};

} // namespace

void launch_rectify_frame(u8 *out, const PackInput *in, const u8 *img, int H, int W, int elem_sz, const float (*rec)[18], int border)
{
    ProfScope p("rectify");
    RectifyRecs r;
    for (int i = 0; i < 18; ++i) {
        r.rec[0][i] = rec[0][i];
        r.rec[1][i] = in ? rec[1][i] : rec[0][i];
    }
    // packed stores where whole pixels may be written: the workspace frame (256-byte aligned) with 3- or 4-byte pixels, and a
    // caller's dword-aligned image of 3-byte pixels
    const bool wide = in ? (elem_sz == 3 || elem_sz == 4) && ((uintptr_t)out & 15) == 0 : elem_sz == 3 && ((uintptr_t)out & 3) == 0;
    dispatch(in, RectifyLaunch{out, make_src(in, img, img, H, W, elem_sz), r, H, W, in ? 1 : 0, in ? 2 * W : W, border, wide ? 1 : 0});
    STM_CHECK_LAUNCH();
}

void launch_rectify_coords(int *quv, int H, int W, const float *rec18)
{
    RectifyRecs r;
    for (int i = 0; i < 18; ++i) r.rec[0][i] = r.rec[1][i] = rec18[i];
    STM_LAUNCH(stm_k_rectify_coords, dim3(cdiv(W, 256), H), dim3(256), 0, stream(), quv, r, H, W);
    STM_CHECK_LAUNCH();
}

} // namespace stm
