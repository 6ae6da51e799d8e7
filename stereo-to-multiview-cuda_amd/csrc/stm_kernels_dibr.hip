// stm_kernels_dibr.hip -- depth-image-based rendering and view multiplexing for gfx950.
//
// Reference stages replaced:
//   demux_sbs                      d_demux_common.cu:8-33
//   dibr_find_occlusion_kernel     d_dibr_occl.cu:114-128   (hit-map scatter)
//   filter_bleed_1_kernel          d_filter.cu:105-139
//   dibr_occl_to_mask_kernel       d_dibr_occl.cu:17-31
//   dibr_backward_warp_kernel x2 + mux_merge_AB_kernel   d_dibr_bwarp.cu:5-22, d_mux_common.cu:23-46
//   dibr_forward_warp_kernel       d_dibr_fwarp.cu:9-25     (deterministic here)
//   mux_multiview_kernel_2 / mux_multiview_kernel        d_mux_multiview.cu:38-84 / :86-124
// The reference synthesises one view with two warp launches, two temporaries and a merge launch;
// here one kernel gathers both sources and blends in registers (same arithmetic, same truncations).
#include "stm_common.h"
#include "stm_views.h"

namespace stm {

// ------------------------------------------------------------------ side-by-side splitter
__global__ __launch_bounds__(256) void stm_k_demux_sbs(u8 *__restrict__ l, u8 *__restrict__ r, const u8 *__restrict__ sbs,
                                                       int H, int Wsbs, int W, int elem_sz)
{
    int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= Wsbs) return;
    const u8 *s = sbs + ((size_t)y * Wsbs + x) * elem_sz;
    u8 *d;
    if (x < W) d = l + ((size_t)y * W + x) * elem_sz;
    else if (x - W < W) d = r + ((size_t)y * W + (x - W)) * elem_sz;
    else return;
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
}
// frame pipeline: the split also emits the two derived pixel formats the disparity stages read, so the frame is
// touched once (requires Wsbs >= 2 W: every pixel of both halves exists)
__global__ __launch_bounds__(256) void stm_k_demux_sbs_packed(u8 *__restrict__ l, u8 *__restrict__ r, uint32_t *__restrict__ pk_l,
                                                              uint32_t *__restrict__ pk_r, uint32_t *__restrict__ wide_l,
                                                              uint32_t *__restrict__ wide_r, const u8 *__restrict__ sbs, int Wsbs,
                                                              int W, int elem_sz)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= 2 * W) return;
    const u8 *s = sbs + ((size_t)y * Wsbs + x) * elem_sz;
    const bool right = x >= W;
    const size_t p = (size_t)y * W + (right ? x - W : x);
    const uint32_t b = s[0], g = s[1], rr = s[2];
    u8 *d = (right ? r : l) + p * elem_sz;
    d[0] = (u8)b; d[1] = (u8)g; d[2] = (u8)rr;
    (right ? pk_r : pk_l)[p] = b | (g << 8) | (rr << 16);
    (right ? wide_r : wide_l)[p] = b | (g << 10) | (rr << 20);
}
void launch_demux_sbs_packed(u8 *l, u8 *r, uint32_t *pk_l, uint32_t *pk_r, uint32_t *wide_l, uint32_t *wide_r, const u8 *sbs, int H,
                             int Wsbs, int W, int elem_sz)
{
    STM_LAUNCH(stm_k_demux_sbs_packed, dim3(cdiv(2 * W, 256), H), dim3(256), 0, stream(), l, r, pk_l, pk_r, wide_l, wide_r,
                       sbs, Wsbs, W, elem_sz);
    STM_CHECK_LAUNCH();
}
void launch_demux_sbs(u8 *l, u8 *r, const u8 *sbs, int H, int Wsbs, int W, int elem_sz)
{
    STM_LAUNCH(stm_k_demux_sbs, dim3(cdiv(Wsbs, 256), H), dim3(256), 0, stream(), l, r, sbs, H, Wsbs, W, elem_sz);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ hit maps ("occlusion")
// occl_r[clamp(x + (int)(dL * 1))] = 1 ; occl_l[clamp(x + (int)(dR * -1))] = 1  (d_dibr_occl.cu:124-127, :156-157)
__global__ __launch_bounds__(256) void stm_k_occl(u8 *__restrict__ occl_l, u8 *__restrict__ occl_r,
                                                  const float *__restrict__ disp_l, const float *__restrict__ disp_r, int H, int W)
{
    int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    size_t row = (size_t)y * W;
    int sd = (int)(disp_l[row + x] * 1.0f); // a caller's map: the conversion saturates, the sum must not wrap (map_col)
    occl_r[row + map_col(x, sd, W)] = 1;
    sd = (int)(disp_r[row + x] * -1.0f);
    occl_l[row + map_col(x, sd, W)] = 1;
}
void launch_occl(u8 *occl_l, u8 *occl_r, const float *disp_l, const float *disp_r, int H, int W)
{
    size_t HW = (size_t)H * W;
    STM_CHECK(hipMemsetAsync(occl_l, 0, HW, stream())); // d_dibr_occl.cu:149-150
    STM_CHECK(hipMemsetAsync(occl_r, 0, HW, stream()));
    STM_LAUNCH(stm_k_occl, dim3(cdiv(W, 256), H), dim3(256), 0, stream(), occl_l, occl_r, disp_l, disp_r, H, W);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ majority dilate ("bleed")
__global__ __launch_bounds__(256) void stm_k_bleed(const u8 *__restrict__ in, u8 *__restrict__ out, int radius, int ksz, int H, int W)
{
    int tx = blockIdx.x * 256 + threadIdx.x, ty = blockIdx.y;
    if (tx >= W) return;
    u8 va = in[(size_t)ty * W + tx];
    int cnt = 0;
    for (int y = -radius; y <= radius; ++y)
        for (int x = -radius; x <= radius; ++x) {
            int sx = tx + x, sy = ty + y;
            if (sx < 0) sx = -sx; // the reference's odd border rule, d_filter.cu:124-127
            if (sy < 0) sy = -sy;
            if (sx > W - 1) sx = W - 1 - x;
            if (sy > H - 1) sy = H - 1 - y;
            sx = min(max(sx, 0), W - 1); sy = min(max(sy, 0), H - 1);
            if (in[(size_t)sy * W + sx] > 0) cnt = cnt + 1;
        }
    out[(size_t)ty * W + tx] = ((double)cnt > (ksz - 1) * 0.30) ? (u8)1 : va;
}
void launch_bleed(const u8 *in, u8 *out, int radius, int H, int W)
{
    int ksz = (2 * radius + 1) * (2 * radius + 1);
    STM_LAUNCH(stm_k_bleed, dim3(cdiv(W, 256), H), dim3(256), 0, stream(), in, out, radius, ksz, H, W);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ 3x3 "median" (d_filter.cu:7-45)
// Samples by flat index without border handling (a step off the row lands in the neighbouring row; an index
// outside the buffer -- an out-of-bounds read in the reference -- is clamped), selection sort on the values
// truncated to int with the truncated values written back by every swap, slot 4 is the result.
__global__ __launch_bounds__(256) void stm_k_median3(const float *__restrict__ in, float *__restrict__ out, int H, int W)
{
    const int tx = blockIdx.x * 256 + threadIdx.x, ty = blockIdx.y;
    if (tx >= W) return;
    const long HW = (long)H * W;
    float v[9];
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        long q = (long)(tx + n % 3 - 1) + (long)(ty + n / 3 - 1) * W;
        q = min(max(q, 0l), HW - 1);
        v[n] = in[q];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        int cur = (int)v[i]; // v_cvt_i32_f32: truncates, saturates, NaN -> 0
#pragma unroll
        for (int j = i; j < 9; ++j) {
            const int comp = (int)v[j];
            if (comp < cur) {
                v[j] = (float)cur;
                v[i] = (float)comp;
                cur = comp;
            }
        }
    }
    out[(size_t)ty * W + tx] = v[4];
}
void launch_median3(const float *in, float *out, int H, int W)
{
    STM_LAUNCH(stm_k_median3, dim3(cdiv(W, 256), H), dim3(256), 0, stream(), in, out, H, W);
    STM_CHECK_LAUNCH();
}

__global__ __launch_bounds__(256) void stm_k_occl_to_mask(float *__restrict__ ml, float *__restrict__ mr,
                                                          const u8 *__restrict__ ol, const u8 *__restrict__ orr, size_t HW)
{
    size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    ml[p] = ol[p] == 1 ? 1.0f : 0.0f;
    mr[p] = orr[p] == 1 ? 1.0f : 0.0f;
}
void launch_occl_to_mask(float *mask_l, float *mask_r, const u8 *occl_l, const u8 *occl_r, int H, int W)
{
    size_t HW = (size_t)H * W;
    STM_LAUNCH(stm_k_occl_to_mask, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, stream(), mask_l, mask_r, occl_l, occl_r, HW);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ hit maps -> bleed(1) -> masks, fused (frame pipeline)
// d_io.cu:165-176 runs dibr_occl, filter_bleed_1(radius 1) on both maps and dibr_occl_to_mask: two zero-fills, the
// scatter, two stencils with a copy back each, the mask kernel.  The scatter never leaves its image row and the
// stencil is 3x3, so one block builds the hit maps of the (at most) three rows its output row reads in LDS, applies
// the majority rule with the reference's border rule and writes both float masks: one launch, no byte planes.
__global__ __launch_bounds__(256) void stm_k_hitmask_rows(float *__restrict__ mask_l, float *__restrict__ mask_r,
                                                          const float *__restrict__ disp_l, const float *__restrict__ disp_r,
                                                          int H, int W)
{
    extern __shared__ u8 hm_lds[]; // [3 rows][left W | right W]
    const int ty = blockIdx.x;
    int src[3]; // image rows behind window rows -1, 0, +1 (d_filter.cu:124-127: sy < 0 -> -sy, sy > H-1 -> H-1-y, then in range)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int y = j - 1;
        int sy = ty + y;
        if (sy < 0) sy = -sy;
        if (sy > H - 1) sy = H - 1 - y;
        src[j] = min(max(sy, 0), H - 1);
    }
    for (int i = threadIdx.x; i < 6 * W; i += 256) hm_lds[i] = 0; // d_dibr_occl.cu:149-150
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        u8 *ol = hm_lds + (size_t)j * 2 * W, *orr = ol + W;
        const size_t row = (size_t)src[j] * W;
        for (int x = threadIdx.x; x < W; x += 256) {
            int sd = (int)(disp_l[row + x] * 1.0f);
            orr[min(max(x + sd, 0), W - 1)] = 1; // d_dibr_occl.cu:124-127
            sd = (int)(disp_r[row + x] * -1.0f);
            ol[min(max(x + sd, 0), W - 1)] = 1;
        }
    }
    __syncthreads();
    const size_t orow = (size_t)ty * W;
    for (int tx = threadIdx.x; tx < W; tx += 256) {
        int cnt_l = 0, cnt_r = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const u8 *ol = hm_lds + (size_t)j * 2 * W, *orr = ol + W;
#pragma unroll
            for (int x = -1; x <= 1; ++x) {
                int sx = tx + x;
                if (sx < 0) sx = -sx;
                if (sx > W - 1) sx = W - 1 - x;
                sx = min(max(sx, 0), W - 1);
                cnt_l += ol[sx] > 0;
                cnt_r += orr[sx] > 0;
            }
        }
        // bleed: count > (9 - 1) * 0.30 -> 1, else the centre value (d_filter.cu:131-137); mask = (value == 1) (d_dibr_occl.cu:17-31)
        const u8 vl = ((double)cnt_l > 8 * 0.30) ? (u8)1 : hm_lds[2 * W + tx];
        const u8 vr = ((double)cnt_r > 8 * 0.30) ? (u8)1 : hm_lds[3 * W + tx];
        mask_l[orow + tx] = vl == 1 ? 1.0f : 0.0f;
        mask_r[orow + tx] = vr == 1 ? 1.0f : 0.0f;
    }
}
void launch_hitmask_rows(float *mask_l, float *mask_r, const float *disp_l, const float *disp_r, int H, int W)
{
    const size_t smem = 6 * (size_t)W;
    if (smem > 64 * 1024) STM_CHECK(hipFuncSetAttribute((const void *)stm_k_hitmask_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    STM_LAUNCH(stm_k_hitmask_rows, dim3(H), dim3(256), smem, stream(), mask_l, mask_r, disp_l, disp_r, H, W);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ one synthesised view
// outL = (u8)(L[sxL] * maskR), sxL = (int)clamp(x + dR * (-shift));  outR = (u8)(R[sxR] * maskL),
// sxR = (int)clamp(x + dL * (1 - shift))   -- the truncation makes alu_bilinear_interp a nearest fetch
// (d_dibr_bwarp.cu:16-21, SURVEY A-Q20);  out = (u8)((1-m) * outL) + (u8)(m * outR), u8 wrap (A-Q22).
//
// One sample of a backward warp: channel c of image row `row` at the clamped position fx in [0, W - 1].
// LINEAR = false: the reference's fetch, img[(int)fx] (the default, bit for bit).
// LINEAR = true (linear sampling, stm_dibr_dbm_lin / frame bit 0x800): alu_bilinear_interp (d_alu.cu:45-71) given the
// untruncated position and cy = (float)y -- the bottom row has weight 0 and is not loaded; x1 = min(x0 + 1, W - 1) keeps the
// second tap inside the row; one f32 operation per line (the file is compiled -ffp-contract=off), (u8) truncates.
template <bool LINEAR>
__device__ __forceinline__ u8 warp_tap(const u8 *__restrict__ img, size_t row, float fx, int c, int W, int elem_sz)
{
    if constexpr (!LINEAR) {
        const int sx = (int)fx;
        return img[(row + sx) * elem_sz + c];
    } else {
        const int x0 = (int)floorf(fx);
        const int x1 = min(x0 + 1, W - 1);
        const float wx = fx - (float)x0;
        const float a = (float)img[(row + x0) * elem_sz + c] * (1.0f - wx);
        const float b = (float)img[(row + x1) * elem_sz + c] * wx;
        const float top = a + b;
        return (u8)top;
    }
}
template <bool LINEAR>
__global__ __launch_bounds__(256) void stm_k_view_synth(u8 *__restrict__ out, const u8 *__restrict__ img_l,
                                                        const u8 *__restrict__ img_r, const float *__restrict__ disp_l,
                                                        const float *__restrict__ disp_r, const float *__restrict__ mask_l,
                                                        const float *__restrict__ mask_r, const float *__restrict__ blend,
                                                        float shift_l, float shift_r, int H, int W, int elem_sz)
{
    int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    size_t row = (size_t)y * W, p = row + x;
    float wmax = (float)(W - 1);
    float sd = disp_r[p] * shift_l;
    float fx = (float)x + sd;
    const float fxl = fminf(fmaxf(fx, 0.0f), wmax);
    sd = disp_l[p] * shift_r;
    fx = (float)x + sd;
    const float fxr = fminf(fmaxf(fx, 0.0f), wmax);
    float vmr = mask_r[p], vml = mask_l[p], m = blend[p];
    float one_m = 1.0f - m;
    u8 *o = out + p * elem_sz;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        u8 a = (u8)((float)warp_tap<LINEAR>(img_l, row, fxl, c, W, elem_sz) * vmr); // left-sourced pixel
        u8 b = (u8)((float)warp_tap<LINEAR>(img_r, row, fxr, c, W, elem_sz) * vml); // right-sourced pixel
        float cb = one_m * (float)a;
        float ca = m * (float)b;
        o[c] = (u8)((u8)cb + (u8)ca);
    }
}
void launch_view_synth(u8 *out, const u8 *img_l, const u8 *img_r, const float *disp_l, const float *disp_r,
                       const float *mask_l, const float *mask_r, const float *blend, float shift, int H, int W, int elem_sz,
                       bool linear)
{
    float shift_l = -shift;                               // d_dibr_bwarp.cu:56
    float shift_r = (float)(1.0 - (double)shift);         // :57
    ProfScope p("view_synth");
    if (linear)
        STM_LAUNCH(stm_k_view_synth<true>, dim3(cdiv(W, 256), H), dim3(256), 0, stream(), out, img_l, img_r, disp_l, disp_r,
                   mask_l, mask_r, blend, shift_l, shift_r, H, W, elem_sz);
    else
        STM_LAUNCH(stm_k_view_synth<false>, dim3(cdiv(W, 256), H), dim3(256), 0, stream(), out, img_l, img_r, disp_l, disp_r,
                   mask_l, mask_r, blend, shift_l, shift_r, H, W, elem_sz);
    STM_CHECK_LAUNCH();
}

// All N-2 synthesised views of a frame in one launch (d_io.cu:186-201 loops over d_dibr_dbm): a thread owns one
// pixel, reads its two disparities, two masks and blend weight once and produces that pixel of every view v = 1..N-2
// with shift = 1 - v / (N - 1) evaluated as the reference does (:189, in double, narrowed).
template <bool LINEAR>
__global__ __launch_bounds__(256) void stm_k_view_synth_all(u8 *__restrict__ views, size_t view_stride, int N,
                                                            const u8 *__restrict__ img_l, const u8 *__restrict__ img_r,
                                                            const float *__restrict__ disp_l, const float *__restrict__ disp_r,
                                                            const float *__restrict__ mask_l, const float *__restrict__ mask_r,
                                                            const float *__restrict__ blend, int H, int W, int elem_sz)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t row = (size_t)y * W, p = row + x;
    const float wmax = (float)(W - 1);
    const float dr = disp_r[p], dl = disp_l[p];
    const float vmr = mask_r[p], vml = mask_l[p], m = blend[p];
    const float one_m = 1.0f - m;
    for (int v = 1; v < N - 1; ++v) {
        const float shift = (float)(1.0 - ((1.0 * (double)(float)v) / ((double)(float)N - 1.0)));
        const float shift_l = -shift;                       // d_dibr_bwarp.cu:56
        const float shift_r = (float)(1.0 - (double)shift); // :57
        float sd = dr * shift_l;
        float fx = (float)x + sd;
        const float fxl = fminf(fmaxf(fx, 0.0f), wmax);
        sd = dl * shift_r;
        fx = (float)x + sd;
        const float fxr = fminf(fmaxf(fx, 0.0f), wmax);
        u8 *o = views + (size_t)v * view_stride + p * elem_sz;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const u8 a = (u8)((float)warp_tap<LINEAR>(img_l, row, fxl, c, W, elem_sz) * vmr);
            const u8 b = (u8)((float)warp_tap<LINEAR>(img_r, row, fxr, c, W, elem_sz) * vml);
            const float cb = one_m * (float)a;
            const float ca = m * (float)b;
            o[c] = (u8)((u8)cb + (u8)ca);
        }
    }
}
// views = base of N view slots of view_stride bytes; slots 1..N-2 are written
void launch_view_synth_all(u8 *views, size_t view_stride, int N, const u8 *img_l, const u8 *img_r, const float *disp_l,
                           const float *disp_r, const float *mask_l, const float *mask_r, const float *blend, int H, int W,
                           int elem_sz, bool linear)
{
    if (N < 3) return;
    ProfScope p("view_synth");
    if (linear)
        STM_LAUNCH(stm_k_view_synth_all<true>, dim3(cdiv(W, 256), H), dim3(256), 0, stream(), views, view_stride, N, img_l, img_r,
                   disp_l, disp_r, mask_l, mask_r, blend, H, W, elem_sz);
    else
        STM_LAUNCH(stm_k_view_synth_all<false>, dim3(cdiv(W, 256), H), dim3(256), 0, stream(), views, view_stride, N, img_l, img_r,
                   disp_l, disp_r, mask_l, mask_r, blend, H, W, elem_sz);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ forward warp (deterministic)
// The reference scatter is a data race (SURVEY A-Q23).  Rule here: of all sources landing on one target
// the LARGEST source x wins, which is what a serial ascending-x loop produces.  Pass 1 resolves the
// winner with atomicMax on a (source x + 1) key per target, pass 2 copies the winner's pixel.
__global__ __launch_bounds__(256) void stm_k_fwarp_vote(const float *__restrict__ disp, float shift,
                                                        unsigned long long *__restrict__ keys, int H, int W)
{
    int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    size_t row = (size_t)y * W;
    int sd = (int)(disp[row + x] * shift); // the f32 product may be +-inf or NaN: saturates / 0, and the sum must not wrap
    int sx = map_col(x, sd, W);
    atomicMax(&keys[row + sx], (unsigned long long)(x + 1));
}
__global__ __launch_bounds__(256) void stm_k_fwarp_copy(u8 *__restrict__ out, const u8 *__restrict__ img,
                                                        const unsigned long long *__restrict__ keys, int H, int W, int elem_sz)
{
    int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    size_t row = (size_t)y * W;
    unsigned long long k = keys[row + x];
    u8 *o = out + (row + x) * elem_sz;
    if (k == 0) { o[0] = 0; o[1] = 0; o[2] = 0; return; } // holes stay 0 (cudaMemset, d_dibr_fwarp.cu:52)
    const u8 *s = img + (row + (size_t)(k - 1)) * elem_sz;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
}
void launch_fwarp(u8 *out, const u8 *img, const float *disp, float shift, unsigned long long *keys, int H, int W, int elem_sz)
{
    STM_CHECK(hipMemsetAsync(keys, 0, (size_t)H * W * 8, stream()));
    STM_LAUNCH(stm_k_fwarp_vote, dim3(cdiv(W, 256), H), dim3(256), 0, stream(), disp, shift, keys, H, W);
    STM_CHECK_LAUNCH();
    STM_LAUNCH(stm_k_fwarp_copy, dim3(cdiv(W, 256), H), dim3(256), 0, stream(), out, img, keys, H, W, elem_sz);
    STM_CHECK_LAUNCH();
}

// table of view pointers for the interlacer: [0] = right image, [N-1] = left image, rest = synthesised
__global__ void stm_k_view_table(u8 **tab, u8 *first, u8 *last, u8 *mem, size_t stride, int N)
{
    int v = threadIdx.x;
    if (v >= N) return;
    tab[v] = v == 0 ? first : (v == N - 1 ? last : mem + (size_t)v * stride);
}
void launch_view_table(u8 **tab, u8 *first, u8 *last, u8 *mem, size_t stride, int N)
{
    STM_LAUNCH(stm_k_view_table, dim3(1), dim3(64 * ((N + 63) / 64)), 0, stream(), tab, first, last, mem, stride, N);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ bilinear resampling (reduced-resolution mode)
__device__ __forceinline__ u8 bilinear_u8(const u8 *__restrict__ data, int elem_sz, int off, float cx, float cy, int width, int height);

// tx_scale_bilinear_kernel, d_tx_scale.cu:30-52
__global__ __launch_bounds__(256) void stm_k_scale_bilinear(const u8 *__restrict__ in, u8 *__restrict__ out, int in_rows,
                                                            int in_cols, int out_rows, int out_cols, int elem_sz)
{
    int gx = blockIdx.x * 256 + threadIdx.x, gy = blockIdx.y;
    if (gx >= out_cols) return;
    float xs = ((float)gx / (float)out_cols) * (float)in_cols;
    xs = fminf(fmaxf(xs, 0.0f), (float)(in_cols - 1));
    float ys = ((float)gy / (float)out_rows) * (float)in_rows;
    ys = fminf(fmaxf(ys, 0.0f), (float)(in_rows - 1));
    size_t o = ((size_t)gx + (size_t)gy * out_cols) * elem_sz;
    out[o + 0] = bilinear_u8(in, elem_sz, 0, xs, ys, in_cols, in_rows);
    out[o + 1] = bilinear_u8(in, elem_sz, 1, xs, ys, in_cols, in_rows);
    out[o + 2] = bilinear_u8(in, elem_sz, 2, xs, ys, in_cols, in_rows);
}
void launch_scale_bilinear(const u8 *in, u8 *out, int in_rows, int in_cols, int out_rows, int out_cols, int elem_sz)
{
    STM_LAUNCH(stm_k_scale_bilinear, dim3(cdiv(out_cols, 256), out_rows), dim3(256), 0, stream(), in, out, in_rows,
                       in_cols, out_rows, out_cols, elem_sz);
    STM_CHECK_LAUNCH();
}

// tx_disp_scale_kernel + alu_bilinear_interp_f, d_tx_scale.cu:8-28, d_alu.cu:17-43
__global__ __launch_bounds__(256) void stm_k_disp_scale(float *__restrict__ out, const float *__restrict__ in, int out_rows,
                                                        int out_cols, int in_rows, int in_cols, float disp_scale)
{
    int tx = blockIdx.x * 256 + threadIdx.x, ty = blockIdx.y;
    if (tx >= out_cols) return;
    float xs = ((float)tx / (float)out_cols) * (float)in_cols;
    xs = fminf(fmaxf(xs, 0.0f), (float)(in_cols - 1));
    float ys = ((float)ty / (float)out_rows) * (float)in_rows;
    ys = fminf(fmaxf(ys, 0.0f), (float)(in_rows - 1));
    int x0 = (int)floorf(xs), y0 = (int)floorf(ys);
    int x1 = min(x0 + 1, in_cols - 1), y1 = min(y0 + 1, in_rows - 1);
    float wx = xs - (float)x0, wy = ys - (float)y0;
    float v00 = in[(size_t)x0 + (size_t)y0 * in_cols], v01 = in[(size_t)x1 + (size_t)y0 * in_cols];
    float v10 = in[(size_t)x0 + (size_t)y1 * in_cols], v11 = in[(size_t)x1 + (size_t)y1 * in_cols];
    float a = v00 * (1.0f - wx);
    float b = v01 * wx;
    float top = a + b;
    a = v10 * (1.0f - wx);
    b = v11 * wx;
    float bot = a + b;
    a = top * (1.0f - wy);
    b = bot * wy;
    float r = a + b;
    out[(size_t)tx + (size_t)ty * out_cols] = r * disp_scale;
}
void launch_disp_scale(float *out, const float *in, int out_rows, int out_cols, int in_rows, int in_cols, float disp_scale)
{
    ProfScope p("disp_scale");
    STM_LAUNCH(stm_k_disp_scale, dim3(cdiv(out_cols, 256), out_rows), dim3(256), 0, stream(), out, in, out_rows, out_cols,
                       in_rows, in_cols, disp_scale);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ multiview interlacer
// fast_bilinear_interp, d_mux_multiview.cu:10-36 (floor, +1 neighbour clamped, u8 truncation)
__device__ __forceinline__ u8 bilinear_u8(const u8 *__restrict__ data, int elem_sz, int off, float cx, float cy, int width, int height)
{
    int x0 = (int)floorf(cx), y0 = (int)floorf(cy);
    int x1 = min(x0 + 1, width - 1), y1 = min(y0 + 1, height - 1);
    float wx = cx - (float)x0, wy = cy - (float)y0;
    float v00 = (float)data[((size_t)x0 + (size_t)y0 * width) * elem_sz + off];
    float v01 = (float)data[((size_t)x1 + (size_t)y0 * width) * elem_sz + off];
    float v10 = (float)data[((size_t)x0 + (size_t)y1 * width) * elem_sz + off];
    float v11 = (float)data[((size_t)x1 + (size_t)y1 * width) * elem_sz + off];
    float a = v00 * (1.0f - wx);
    float b = v01 * wx;
    float top = a + b;
    a = v10 * (1.0f - wx);
    b = v11 * wx;
    float bot = a + b;
    a = top * (1.0f - wy);
    b = bot * wy;
    return (u8)(a + b);
}

__global__ __launch_bounds__(256) void stm_k_mux(const u8 *const *__restrict__ views, u8 *__restrict__ out, int N,
                                                 float y_interval, float inv_y, int ymod, int Hin, int Win, int Hout,
                                                 int Wout, int elem_sz, int variant)
{
    int tx = blockIdx.x * 256 + threadIdx.x, ty = blockIdx.y;
    if (tx >= Wout) return;
    float xs = ((float)tx / (float)Wout) * (float)Win;
    xs = fminf(fmaxf(xs, 0.0f), (float)(Win - 1));
    float ys = ((float)ty / (float)Hout) * (float)Hin;
    ys = fminf(fmaxf(ys, 0.0f), (float)(Hin - 1));
    int r_view = mux_r_view(tx, ty, N, y_interval, inv_y, ymod, variant); // :62-63 vs :105-106
    int g_view = r_view + 1, b_view = r_view + 2;
    if (g_view >= N) g_view -= N;
    if (b_view >= N) b_view -= N;
    size_t o = ((size_t)tx + (size_t)ty * Wout) * elem_sz;
    out[o + 0] = bilinear_u8(views[b_view], elem_sz, 0, xs, ys, Win, Hin);
    out[o + 1] = bilinear_u8(views[g_view], elem_sz, 1, xs, ys, Win, Hin);
    out[o + 2] = bilinear_u8(views[r_view], elem_sz, 2, xs, ys, Win, Hin);
}
// ------------------------------------------------------------------ view synthesis + interlacing in one pass (frame pipeline)
// The frame pipeline used to write the N - 2 synthesised views (stm_k_view_synth_all: 37 MB at 1080p, 8 views) only for the
// interlacer to pick ONE channel of THREE views per output pixel out of them (stm_k_mux).  Here an output pixel synthesises
// exactly the samples it interlaces: per channel the view v = r, r + 1, r + 2 (mod N) of mux_multiview_kernel_2
// (d_mux_multiview.cu:60-73) at the up to four neighbours of fast_bilinear_interp (:10-36) -- a neighbour whose weight is
// exactly 0 is not evaluated (v * 0 = +0 and a + 0 = a for the finite, non-negative values involved: same result) -- each one
// computed as d_dibr_dbm does (backward warp of both images, masks, blend: d_dibr_bwarp.cu:5-70, d_mux_common.cu:23-46), with
// view 0 = the right image and view N - 1 = the left image (d_io.cu:182-183).  Same arithmetic, no view buffers.
struct SynthArgs {
    const u8 *img_l, *img_r;
    const float *disp_l, *disp_r, *mask_l, *mask_r, *blend;
};
template <bool LINEAR>
__device__ __forceinline__ u8 synth_sample(const SynthArgs &a, int N, int v, int c, int x, int y, int W, int elem_sz)
{
    const size_t row = (size_t)y * W, p = row + x;
    if (v == 0) return a.img_r[p * elem_sz + c];
    if (v == N - 1) return a.img_l[p * elem_sz + c];
    const float wmax = (float)(W - 1);
    const float shift = (float)(1.0 - ((1.0 * (double)(float)v) / ((double)(float)N - 1.0))); // d_io.cu:189
    const float shift_l = -shift;                       // d_dibr_bwarp.cu:56
    const float shift_r = (float)(1.0 - (double)shift); // :57
    float sd = a.disp_r[p] * shift_l;
    float fx = (float)x + sd;
    const float fxl = fminf(fmaxf(fx, 0.0f), wmax);
    sd = a.disp_l[p] * shift_r;
    fx = (float)x + sd;
    const float fxr = fminf(fmaxf(fx, 0.0f), wmax);
    const float m = a.blend[p], one_m = 1.0f - m;
    const u8 pa = (u8)((float)warp_tap<LINEAR>(a.img_l, row, fxl, c, W, elem_sz) * a.mask_r[p]); // left-sourced pixel
    const u8 pb = (u8)((float)warp_tap<LINEAR>(a.img_r, row, fxr, c, W, elem_sz) * a.mask_l[p]); // right-sourced pixel
    const float cb = one_m * (float)pa;
    const float ca = m * (float)pb;
    return (u8)((u8)cb + (u8)ca);
}
template <bool LINEAR>
__device__ __forceinline__ u8 synth_bilinear(const SynthArgs &a, int N, int v, int c, float cx, float cy, int W, int H, int elem_sz)
{
    const int x0 = (int)floorf(cx), y0 = (int)floorf(cy);
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float wx = cx - (float)x0, wy = cy - (float)y0;
    const float v00 = (float)synth_sample<LINEAR>(a, N, v, c, x0, y0, W, elem_sz);
    const float v01 = wx != 0.0f ? (float)synth_sample<LINEAR>(a, N, v, c, x1, y0, W, elem_sz) : 0.0f;
    float ta = v00 * (1.0f - wx);
    float tb = v01 * wx;
    const float top = ta + tb;
    float bot = 0.0f;
    if (wy != 0.0f) {
        const float v10 = (float)synth_sample<LINEAR>(a, N, v, c, x0, y1, W, elem_sz);
        const float v11 = wx != 0.0f ? (float)synth_sample<LINEAR>(a, N, v, c, x1, y1, W, elem_sz) : 0.0f;
        ta = v10 * (1.0f - wx);
        tb = v11 * wx;
        bot = ta + tb;
    }
    ta = top * (1.0f - wy);
    tb = bot * wy;
    return (u8)(ta + tb);
}
template <bool LINEAR>
__global__ __launch_bounds__(256) void stm_k_synth_mux(SynthArgs a, u8 *__restrict__ out, int N, float y_interval, float inv_y, int ymod,
                                                       int Hin, int Win, int Hout, int Wout, int elem_sz, int variant)
{
    const int tx = blockIdx.x * 256 + threadIdx.x, ty = blockIdx.y;
    if (tx >= Wout) return;
    float xs = ((float)tx / (float)Wout) * (float)Win;
    xs = fminf(fmaxf(xs, 0.0f), (float)(Win - 1));
    float ys = ((float)ty / (float)Hout) * (float)Hin;
    ys = fminf(fmaxf(ys, 0.0f), (float)(Hin - 1));
    const int r_view = mux_r_view(tx, ty, N, y_interval, inv_y, ymod, variant); // d_mux_multiview.cu:62-63 vs :105-106
    int g_view = r_view + 1, b_view = r_view + 2;
    if (g_view >= N) g_view -= N;
    if (b_view >= N) b_view -= N;
    const size_t o = ((size_t)tx + (size_t)ty * Wout) * elem_sz;
    out[o + 0] = synth_bilinear<LINEAR>(a, N, b_view, 0, xs, ys, Win, Hin, elem_sz);
    out[o + 1] = synth_bilinear<LINEAR>(a, N, g_view, 1, xs, ys, Win, Hin, elem_sz);
    out[o + 2] = synth_bilinear<LINEAR>(a, N, r_view, 2, xs, ys, Win, Hin, elem_sz);
}
void launch_synth_mux(const u8 *img_l, const u8 *img_r, const float *disp_l, const float *disp_r, const float *mask_l, const float *mask_r,
                      const float *blend, u8 *out, int N, float y_interval, float inv_y_interval, int ymod, int Hin, int Win, int Hout,
                      int Wout, int elem_sz, int variant, bool linear)
{
    SynthArgs a{img_l, img_r, disp_l, disp_r, mask_l, mask_r, blend};
    ProfScope p("synth_mux");
    if (linear)
        STM_LAUNCH(stm_k_synth_mux<true>, dim3(cdiv(Wout, 256), Hout), dim3(256), 0, stream(), a, out, N, y_interval, inv_y_interval,
                   ymod, Hin, Win, Hout, Wout, elem_sz, variant);
    else
        STM_LAUNCH(stm_k_synth_mux<false>, dim3(cdiv(Wout, 256), Hout), dim3(256), 0, stream(), a, out, N, y_interval, inv_y_interval,
                   ymod, Hin, Win, Hout, Wout, elem_sz, variant);
    STM_CHECK_LAUNCH();
}

void launch_mux(const u8 *const *d_views, u8 *out, int N, float y_interval, float inv_y_interval, int ymod, int Hin,
                int Win, int Hout, int Wout, int elem_sz, int variant)
{
    ProfScope p("mux");
    STM_LAUNCH(stm_k_mux, dim3(cdiv(Wout, 256), Hout), dim3(256), 0, stream(), d_views, out, N, y_interval,
                       inv_y_interval, ymod, Hin, Win, Hout, Wout, elem_sz, variant);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ calibrated lenticular interlacing (stm_hip.h, stm_set_lens)
// mux_multiview_kernel_2 takes a sub-pixel's view from (3 tx + int((ty % round(yi) + 1) N / yi)) % N: a lens pitch of exactly N
// sub-pixels, no phase offset, a slant whose row period is rounded to an integer.  Here the view follows from the panel's
// calibration: the lens phase of sub-pixel k = 2 - c of output pixel (tx, ty), in double, one operation per line (the file is
// compiled -ffp-contract=off and the f64 division is the correctly rounded one).  The sampling position (xs, ys) and the
// 4-neighbour sampler stay the reference's.  lens_phase and lens_pick live in stm_views.h: the overlay compositor shares them.
template <int MODE>
__global__ __launch_bounds__(256) void stm_k_mux_lens(const u8 *const *__restrict__ views, u8 *__restrict__ out, int N, Lens g, int Hin,
                                                      int Win, int Hout, int Wout, int elem_sz)
{
    const int tx = blockIdx.x * 256 + threadIdx.x, ty = blockIdx.y;
    if (tx >= Wout) return;
    float xs = ((float)tx / (float)Wout) * (float)Win;
    xs = fminf(fmaxf(xs, 0.0f), (float)(Win - 1));
    float ys = ((float)ty / (float)Hout) * (float)Hin;
    ys = fminf(fmaxf(ys, 0.0f), (float)(Hin - 1));
    const size_t o = ((size_t)tx + (size_t)ty * Wout) * elem_sz;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int v;
        float w, shift;
        lens_pick<MODE>(lens_phase(tx, ty, c, g), N, v, w, shift);
        const u8 A = bilinear_u8(views[v], elem_sz, c, xs, ys, Win, Hin);
        if constexpr (MODE == 1) {
            out[o + c] = A;
        } else {
            const u8 B = bilinear_u8(views[v + 1], elem_sz, c, xs, ys, Win, Hin);
            const float p = (float)A * (1.0f - w);
            const float q = (float)B * w;
            out[o + c] = (u8)(p + q);
        }
    }
}
void launch_mux_lens(const u8 *const *d_views, u8 *out, int N, const Lens &ln, int Hin, int Win, int Hout, int Wout, int elem_sz)
{
    ProfScope p("mux");
    if (ln.mode == 1)
        STM_LAUNCH(stm_k_mux_lens<1>, dim3(cdiv(Wout, 256), Hout), dim3(256), 0, stream(), d_views, out, N, ln, Hin, Win, Hout, Wout, elem_sz);
    else
        STM_LAUNCH(stm_k_mux_lens<2>, dim3(cdiv(Wout, 256), Hout), dim3(256), 0, stream(), d_views, out, N, ln, Hin, Win, Hout, Wout, elem_sz);
    STM_CHECK_LAUNCH();
}

// The fused renderer under a lens geometry: stm_k_synth_mux with each sub-pixel's view -- or, in mode 3, its own shift -- taken
// from the lens phase.  One thread per output pixel; what a neighbour contributes besides the two warped colours (its two
// disparities, two masks and blend weight) is loaded once and serves the three channels.
struct LensNb {
    size_t row;
    int x;
    float dl, dr, ml, mr, m;
};
__device__ __forceinline__ LensNb lens_nb(const SynthArgs &a, int x, int y, int W)
{
    LensNb n;
    n.row = (size_t)y * W;
    n.x = x;
    const size_t p = n.row + x;
    n.dl = a.disp_l[p]; n.dr = a.disp_r[p];
    n.ml = a.mask_l[p]; n.mr = a.mask_r[p];
    n.m = a.blend[p];
    return n;
}
// synth_sample's general branch at an arbitrary shift (no end-view shortcut)
template <bool LINEAR>
__device__ __forceinline__ u8 lens_sample_shift(const SynthArgs &a, const LensNb &n, float shift, int c, int W, int elem_sz)
{
    const float wmax = (float)(W - 1);
    const float shift_l = -shift;                       // d_dibr_bwarp.cu:56
    const float shift_r = (float)(1.0 - (double)shift); // :57
    float sd = n.dr * shift_l;
    float fx = (float)n.x + sd;
    const float fxl = fminf(fmaxf(fx, 0.0f), wmax);
    sd = n.dl * shift_r;
    fx = (float)n.x + sd;
    const float fxr = fminf(fmaxf(fx, 0.0f), wmax);
    const float one_m = 1.0f - n.m;
    const u8 pa = (u8)((float)warp_tap<LINEAR>(a.img_l, n.row, fxl, c, W, elem_sz) * n.mr); // left-sourced pixel
    const u8 pb = (u8)((float)warp_tap<LINEAR>(a.img_r, n.row, fxr, c, W, elem_sz) * n.ml); // right-sourced pixel
    const float cb = one_m * (float)pa;
    const float ca = n.m * (float)pb;
    return (u8)((u8)cb + (u8)ca);
}
// CONTINUOUS = false: synth_sample of the discrete view v; true: the sample at `shift`
template <bool LINEAR, bool CONTINUOUS>
__device__ __forceinline__ u8 lens_sample(const SynthArgs &a, const LensNb &n, int N, int v, float shift, int c, int W, int elem_sz)
{
    if constexpr (!CONTINUOUS) {
        if (v == 0) return a.img_r[(n.row + n.x) * elem_sz + c];
        if (v == N - 1) return a.img_l[(n.row + n.x) * elem_sz + c];
        shift = (float)(1.0 - ((1.0 * (double)(float)v) / ((double)(float)N - 1.0))); // d_io.cu:189
    }
    return lens_sample_shift<LINEAR>(a, n, shift, c, W, elem_sz);
}
// synth_bilinear on the loaded neighbours (a neighbour of weight exactly 0 is not evaluated)
template <bool LINEAR, bool CONTINUOUS>
__device__ __forceinline__ u8 lens_bilinear(const SynthArgs &a, const LensNb &n00, const LensNb &n01, const LensNb &n10, const LensNb &n11,
                                            float wx, float wy, int N, int v, float shift, int c, int W, int elem_sz)
{
    const float v00 = (float)lens_sample<LINEAR, CONTINUOUS>(a, n00, N, v, shift, c, W, elem_sz);
    const float v01 = wx != 0.0f ? (float)lens_sample<LINEAR, CONTINUOUS>(a, n01, N, v, shift, c, W, elem_sz) : 0.0f;
    float ta = v00 * (1.0f - wx);
    float tb = v01 * wx;
    const float top = ta + tb;
    float bot = 0.0f;
    if (wy != 0.0f) {
        const float v10 = (float)lens_sample<LINEAR, CONTINUOUS>(a, n10, N, v, shift, c, W, elem_sz);
        const float v11 = wx != 0.0f ? (float)lens_sample<LINEAR, CONTINUOUS>(a, n11, N, v, shift, c, W, elem_sz) : 0.0f;
        ta = v10 * (1.0f - wx);
        tb = v11 * wx;
        bot = ta + tb;
    }
    ta = top * (1.0f - wy);
    tb = bot * wy;
    return (u8)(ta + tb);
}
template <int MODE, bool LINEAR>
__global__ __launch_bounds__(256) void stm_k_synth_mux_lens(SynthArgs a, u8 *__restrict__ out, int N, Lens g, int Hin, int Win, int Hout,
                                                            int Wout, int elem_sz)
{
    const int tx = blockIdx.x * 256 + threadIdx.x, ty = blockIdx.y;
    if (tx >= Wout) return;
    float xs = ((float)tx / (float)Wout) * (float)Win;
    xs = fminf(fmaxf(xs, 0.0f), (float)(Win - 1));
    float ys = ((float)ty / (float)Hout) * (float)Hin;
    ys = fminf(fmaxf(ys, 0.0f), (float)(Hin - 1));
    const int x0 = (int)floorf(xs), y0 = (int)floorf(ys);
    const int x1 = min(x0 + 1, Win - 1), y1 = min(y0 + 1, Hin - 1);
    const float wx = xs - (float)x0, wy = ys - (float)y0;
    const LensNb n00 = lens_nb(a, x0, y0, Win);
    LensNb n01 = n00, n10 = n00, n11 = n00; // only read where the weight is not 0
    if (wx != 0.0f) n01 = lens_nb(a, x1, y0, Win);
    if (wy != 0.0f) {
        n10 = lens_nb(a, x0, y1, Win);
        if (wx != 0.0f) n11 = lens_nb(a, x1, y1, Win);
    }
    const size_t o = ((size_t)tx + (size_t)ty * Wout) * elem_sz;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int v;
        float w, shift;
        lens_pick<MODE>(lens_phase(tx, ty, c, g), N, v, w, shift);
        if constexpr (MODE == 3) {
            out[o + c] = lens_bilinear<LINEAR, true>(a, n00, n01, n10, n11, wx, wy, N, 0, shift, c, Win, elem_sz);
        } else {
            const u8 A = lens_bilinear<LINEAR, false>(a, n00, n01, n10, n11, wx, wy, N, v, 0.0f, c, Win, elem_sz);
            if constexpr (MODE == 1) {
                out[o + c] = A;
            } else {
                const u8 B = lens_bilinear<LINEAR, false>(a, n00, n01, n10, n11, wx, wy, N, v + 1, 0.0f, c, Win, elem_sz);
                const float p = (float)A * (1.0f - w);
                const float q = (float)B * w;
                out[o + c] = (u8)(p + q);
            }
        }
    }
}
template <int MODE>
static void launch_synth_mux_lens_mode(const SynthArgs &a, u8 *out, int N, const Lens &ln, int Hin, int Win, int Hout, int Wout,
                                       int elem_sz, bool linear)
{
    if (linear)
        STM_LAUNCH((stm_k_synth_mux_lens<MODE, true>), dim3(cdiv(Wout, 256), Hout), dim3(256), 0, stream(), a, out, N, ln, Hin, Win, Hout,
                   Wout, elem_sz);
    else
        STM_LAUNCH((stm_k_synth_mux_lens<MODE, false>), dim3(cdiv(Wout, 256), Hout), dim3(256), 0, stream(), a, out, N, ln, Hin, Win, Hout,
                   Wout, elem_sz);
}
void launch_synth_mux_lens(const u8 *img_l, const u8 *img_r, const float *disp_l, const float *disp_r, const float *mask_l,
                           const float *mask_r, const float *blend, u8 *out, int N, const Lens &ln, int Hin, int Win, int Hout, int Wout,
                           int elem_sz, bool linear)
{
    SynthArgs a{img_l, img_r, disp_l, disp_r, mask_l, mask_r, blend};
    ProfScope p("synth_mux");
    if (ln.mode == 1) launch_synth_mux_lens_mode<1>(a, out, N, ln, Hin, Win, Hout, Wout, elem_sz, linear);
    else if (ln.mode == 2) launch_synth_mux_lens_mode<2>(a, out, N, ln, Hin, Win, Hout, Wout, elem_sz, linear);
    else launch_synth_mux_lens_mode<3>(a, out, N, ln, Hin, Win, Hout, Wout, elem_sz, linear);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ depth budget (stm_hip.h, stm_set_depth)
// The fused renderer with a view's position s mapped to the shift it is rendered at and to a horizontal offset of its sampling
// position: s2 = 0.5 + gain (s - 0.5), cx = clamp(xs + conv (s - 0.5)).  Every sample takes the general form at s2 (no end-view
// shortcut: at gain != 1 the end views are warps too).  LMODE 0 = the reference's view assignment, 1 .. 3 = the lens modes.
// (view_shift and MuxGeom: stm_views.h.)
// the four neighbours of the position a sample is taken at.  The three channels of a pixel belong to three views, so with
// conv != 0 their positions differ; where two of them share x0 (always, with conv == 0) the neighbours' maps are loaded once.
struct DepthNbs {
    int x0;
    bool has_x1;
    LensNb n00, n01, n10, n11;
};
template <bool LINEAR>
__device__ __forceinline__ u8 depth_sample(const SynthArgs &a, DepthNbs &nb, float s, float xs, int y0, int y1, float wy, float gain,
                                           float conv, int c, int Win, int elem_sz)
{
    const double t = (double)s - 0.5;
    double u = (double)gain * t;
    const float s2 = (float)(0.5 + u);
    u = (double)conv * t;
    const float off = (float)u;
    float cx = xs + off;
    cx = fminf(fmaxf(cx, 0.0f), (float)(Win - 1)); // C fmaxf: a NaN becomes 0
    const int x0 = (int)floorf(cx);
    const int x1 = min(x0 + 1, Win - 1);
    const float wx = cx - (float)x0;
    if (x0 != nb.x0 || (wx != 0.0f && !nb.has_x1)) { // only read where the weight is not 0
        nb.x0 = x0;
        nb.has_x1 = wx != 0.0f;
        nb.n00 = lens_nb(a, x0, y0, Win);
        nb.n01 = nb.n10 = nb.n11 = nb.n00;
        if (wx != 0.0f) nb.n01 = lens_nb(a, x1, y0, Win);
        if (wy != 0.0f) {
            nb.n10 = lens_nb(a, x0, y1, Win);
            if (wx != 0.0f) nb.n11 = lens_nb(a, x1, y1, Win);
        }
    }
    return lens_bilinear<LINEAR, true>(a, nb.n00, nb.n01, nb.n10, nb.n11, wx, wy, 0, 0, s2, c, Win, elem_sz);
}
template <int LMODE, bool LINEAR>
__global__ __launch_bounds__(256) void stm_k_synth_mux_depth(SynthArgs a, u8 *__restrict__ out, int N, MuxGeom mg, Lens g, float gain,
                                                             float conv, const float *__restrict__ state, int Hin, int Win, int Hout,
                                                             int Wout, int elem_sz)
{
    const int tx = blockIdx.x * 256 + threadIdx.x, ty = blockIdx.y;
    if (tx >= Wout) return;
    if (state) { // automatic mode: what stm_k_depth_fit left for this frame
        gain = state[1];
        conv = state[2];
    }
    float xs = ((float)tx / (float)Wout) * (float)Win;
    xs = fminf(fmaxf(xs, 0.0f), (float)(Win - 1));
    float ys = ((float)ty / (float)Hout) * (float)Hin;
    ys = fminf(fmaxf(ys, 0.0f), (float)(Hin - 1));
    const int y0 = (int)floorf(ys);
    const int y1 = min(y0 + 1, Hin - 1);
    const float wy = ys - (float)y0;
    int r_view = 0;
    if constexpr (LMODE == 0) r_view = mux_r_view(tx, ty, N, 0.0f, mg.inv_y, mg.ymod, 2); // d_mux_multiview.cu:62-63
    DepthNbs nb;
    nb.x0 = -1;
    nb.has_x1 = false;
    const size_t o = ((size_t)tx + (size_t)ty * Wout) * elem_sz;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (LMODE == 0) {
            int v = r_view + (2 - c); // byte 0 = the b view (r + 2), byte 2 = the r view
            if (v >= N) v -= N;
            out[o + c] = depth_sample<LINEAR>(a, nb, view_shift(v, N), xs, y0, y1, wy, gain, conv, c, Win, elem_sz);
        } else {
            int v;
            float w, shift;
            lens_pick<LMODE>(lens_phase(tx, ty, c, g), N, v, w, shift);
            if constexpr (LMODE == 3) {
                out[o + c] = depth_sample<LINEAR>(a, nb, shift, xs, y0, y1, wy, gain, conv, c, Win, elem_sz);
            } else {
                const u8 A = depth_sample<LINEAR>(a, nb, view_shift(v, N), xs, y0, y1, wy, gain, conv, c, Win, elem_sz);
                if constexpr (LMODE == 1) {
                    out[o + c] = A;
                } else {
                    const u8 B = depth_sample<LINEAR>(a, nb, view_shift(v + 1, N), xs, y0, y1, wy, gain, conv, c, Win, elem_sz);
                    const float p = (float)A * (1.0f - w);
                    const float q = (float)B * w;
                    out[o + c] = (u8)(p + q);
                }
            }
        }
    }
}
template <int LMODE>
static void launch_synth_mux_depth_mode(const SynthArgs &a, u8 *out, int N, const MuxGeom &mg, const Lens &ln, float gain, float conv,
                                        const float *state, int Hin, int Win, int Hout, int Wout, int elem_sz, bool linear)
{
    if (linear)
        STM_LAUNCH((stm_k_synth_mux_depth<LMODE, true>), dim3(cdiv(Wout, 256), Hout), dim3(256), 0, stream(), a, out, N, mg, ln, gain, conv,
                   state, Hin, Win, Hout, Wout, elem_sz);
    else
        STM_LAUNCH((stm_k_synth_mux_depth<LMODE, false>), dim3(cdiv(Wout, 256), Hout), dim3(256), 0, stream(), a, out, N, mg, ln, gain, conv,
                   state, Hin, Win, Hout, Wout, elem_sz);
}
// ln.mode 0: the reference's assignment from inv_y_interval and ymod; state != nullptr: gain and conv are read from state[1], state[2]
void launch_synth_mux_depth(const u8 *img_l, const u8 *img_r, const float *disp_l, const float *disp_r, const float *mask_l,
                            const float *mask_r, const float *blend, u8 *out, int N, const Lens &ln, float inv_y_interval, int ymod,
                            float gain, float conv, const float *state, int Hin, int Win, int Hout, int Wout, int elem_sz, bool linear)
{
    SynthArgs a{img_l, img_r, disp_l, disp_r, mask_l, mask_r, blend};
    const MuxGeom mg{inv_y_interval, ymod};
    ProfScope p("synth_mux");
    if (ln.mode == 0) launch_synth_mux_depth_mode<0>(a, out, N, mg, ln, gain, conv, state, Hin, Win, Hout, Wout, elem_sz, linear);
    else if (ln.mode == 1) launch_synth_mux_depth_mode<1>(a, out, N, mg, ln, gain, conv, state, Hin, Win, Hout, Wout, elem_sz, linear);
    else if (ln.mode == 2) launch_synth_mux_depth_mode<2>(a, out, N, mg, ln, gain, conv, state, Hin, Win, Hout, Wout, elem_sz, linear);
    else launch_synth_mux_depth_mode<3>(a, out, N, mg, ln, gain, conv, state, Hin, Win, Hout, Wout, elem_sz, linear);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ quilt output (stm_hip.h, stm_set_layout)
// The views as a grid of tiles instead of interlaced sub-pixels: view v fills tile k = (order & 2) ? N - 1 - v : v of tiles_x x
// tiles_y tiles of tw x th pixels, each tile the whole view resampled -- by the reference's four-neighbour sampler (filter 0) or by
// the exact area average (filter 1).  A view's pixel V(v, x, y, c) comes from one of three sources:
//   QSRC_VIEWS  a table of finished views (the stage stm_quilt_multiview, and the frame under stm_set_agg_variant(200))
//   QSRC_SYNTH  the frame's renderer, synth_sample (the end views are the two images)
//   QSRC_DEPTH  the renderer under a depth budget, depth_sample at s = view_shift(v, N), xs = (float)x, y0 = y1 = y, wy = 0
// so the fused kernels write no view to memory.
enum { QSRC_VIEWS = 0, QSRC_SYNTH = 1, QSRC_DEPTH = 2, QSRC_IMAGE = 3 }; // QSRC_IMAGE (inside the kernels): an end view of QSRC_SYNTH
struct QuiltSrc {
    const u8 *image;        // QSRC_IMAGE
    const u8 *const *views; // QSRC_VIEWS
    SynthArgs a;            // QSRC_SYNTH, QSRC_DEPTH
    float gain, conv;       // QSRC_DEPTH
    const float *state;     // QSRC_DEPTH, automatic mode: gain and conv are read from state[1], state[2]
};
// (QuiltGeom and quilt_tile_origin: stm_views.h)
// the three channels of V(v, x, y): the maps of the pixel are loaded once
template <int SRC, bool LINEAR>
__device__ __forceinline__ void quilt_render3(const QuiltSrc &s, const QuiltGeom &g, int v, int x, int y, uint32_t (&px)[3])
{
    if constexpr (SRC == QSRC_VIEWS || SRC == QSRC_IMAGE) {
        const u8 *p = (SRC == QSRC_VIEWS ? s.views[v] : s.image) + ((size_t)y * g.Win + x) * g.elem_sz;
        px[0] = p[0]; px[1] = p[1]; px[2] = p[2];
    } else if constexpr (SRC == QSRC_SYNTH) { // an interior view (the callers take the end views as QSRC_IMAGE): synth_sample's general branch
        const LensNb n = lens_nb(s.a, x, y, g.Win);
        const float sh = view_shift(v, g.N);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = lens_sample_shift<LINEAR>(s.a, n, sh, c, g.Win, g.elem_sz);
    } else {
        DepthNbs nb;
        nb.x0 = -1;
        nb.has_x1 = false;
        const float sh = view_shift(v, g.N);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = depth_sample<LINEAR>(s.a, nb, sh, (float)x, y, y, 0.0f, s.gain, s.conv, c, g.Win, g.elem_sz);
    }
}
// the overlap of output interval u with source interval x in units of 1 / t of a source pixel (t = the tile's size, n = the view's)
__device__ __forceinline__ uint32_t quilt_weight(int u, int x, int n, int t)
{
    const int lo = max(u * n, x * t), hi = min((u + 1) * n, (x + 1) * t);
    return (uint32_t)max(hi - lo, 0);
}
__device__ __forceinline__ u8 quilt_round(unsigned long long acc, const QuiltGeom &g)
{
    const unsigned long long den = (unsigned long long)g.Win * (unsigned long long)g.Hin;
    if (g.narrow) return (u8)(((uint32_t)acc + (uint32_t)den / 2u) / (uint32_t)den);
    return (u8)((acc + den / 2) / den);
}

// The pixels that belong to no tile: the remainder columns at the right over every row, then the remainder rows over the tiles'
// columns.  Their first three bytes are written 0.
__global__ __launch_bounds__(256) void stm_k_quilt_pad(u8 *__restrict__ out, QuiltGeom g, int rem_w, int rem_h)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n_right = (size_t)rem_w * g.Hout, used_w = (size_t)(g.Wout - rem_w);
    int x, y;
    if (t < n_right) {
        y = (int)(t / rem_w);
        x = (int)used_w + (int)(t - (size_t)y * rem_w);
    } else {
        const size_t q = t - n_right;
        if (q >= used_w * rem_h) return;
        const int r = (int)(q / used_w);
        x = (int)(q - (size_t)r * used_w);
        y = (g.order & 1) ? r : g.Hout - rem_h + r; // bottom-up tiles leave the top rows
    }
    u8 *o = out + ((size_t)y * g.Wout + x) * g.elem_sz;
    o[0] = 0; o[1] = 0; o[2] = 0;
}

// Filter 0, one thread per output pixel: stm_k_mux's sampling position with the tile's size in place of the frame's, the
// four-neighbour sampler on the renderer's samples.  The pixels outside every tile are written here.
template <int SRC, bool LINEAR>
__global__ __launch_bounds__(256) void stm_k_quilt_nb(QuiltSrc s, u8 *__restrict__ out, QuiltGeom g)
{
    const int tx = blockIdx.x * 256 + threadIdx.x, ty = blockIdx.y;
    if (tx >= g.Wout) return;
    if constexpr (SRC == QSRC_DEPTH)
        if (s.state) { // automatic mode: what stm_k_depth_fit left for this frame
            s.gain = s.state[1];
            s.conv = s.state[2];
        }
    u8 *o = out + ((size_t)tx + (size_t)ty * g.Wout) * g.elem_sz;
    const int i = tx / g.tw;
    const int r = (g.order & 1) ? g.Hout - 1 - ty : ty; // rows counted from the edge the tile rows start at
    const int j = r / g.th;
    if (i >= g.tiles_x || j >= g.tiles_y) {
        o[0] = 0; o[1] = 0; o[2] = 0;
        return;
    }
    const int k = j * g.tiles_x + i;
    const int v = (g.order & 2) ? g.N - 1 - k : k;
    int left, top;
    quilt_tile_origin(g, k, left, top);
    const int u = tx - left, w = ty - top;
    float xs = ((float)u / (float)g.tw) * (float)g.Win;
    xs = fminf(fmaxf(xs, 0.0f), (float)(g.Win - 1));
    float ys = ((float)w / (float)g.th) * (float)g.Hin;
    ys = fminf(fmaxf(ys, 0.0f), (float)(g.Hin - 1));
    if constexpr (SRC == QSRC_VIEWS) {
        const u8 *vw = s.views[v];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = bilinear_u8(vw, g.elem_sz, c, xs, ys, g.Win, g.Hin);
    } else {
        const int y0 = (int)floorf(ys);
        const int y1 = min(y0 + 1, g.Hin - 1);
        const float wy = ys - (float)y0;
        if constexpr (SRC == QSRC_SYNTH) {
            const int x0 = (int)floorf(xs);
            const int x1 = min(x0 + 1, g.Win - 1);
            const float wx = xs - (float)x0;
            const LensNb n00 = lens_nb(s.a, x0, y0, g.Win);
            LensNb n01 = n00, n10 = n00, n11 = n00; // only read where the weight is not 0
            if (wx != 0.0f) n01 = lens_nb(s.a, x1, y0, g.Win);
            if (wy != 0.0f) {
                n10 = lens_nb(s.a, x0, y1, g.Win);
                if (wx != 0.0f) n11 = lens_nb(s.a, x1, y1, g.Win);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = lens_bilinear<LINEAR, false>(s.a, n00, n01, n10, n11, wx, wy, g.N, v, 0.0f, c, g.Win, g.elem_sz);
        } else {
            DepthNbs nb;
            nb.x0 = -1;
            nb.has_x1 = false;
            const float sh = view_shift(v, g.N);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = depth_sample<LINEAR>(s.a, nb, sh, xs, y0, y1, wy, s.gain, s.conv, c, g.Win, g.elem_sz);
        }
    }
}

// The staging of stm_k_quilt_area: the fw x fh view pixels from (fx0, fy0) rendered into pix, QUILT_STAGE_UNROLL independent pixels
// per thread and step so that their loads are in flight together (a step past the end renders the last pixel again and stores nothing)
#define QUILT_STAGE_UNROLL 4
template <int SRC, bool LINEAR>
__device__ __forceinline__ void quilt_stage(const QuiltSrc &s, const QuiltGeom &g, int v, int fx0, int fy0, int fw, int fh, uint32_t *pix)
{
    const int n = fw * fh;
    for (int t0 = threadIdx.x; t0 < n; t0 += 256 * QUILT_STAGE_UNROLL) {
        uint32_t r[QUILT_STAGE_UNROLL];
#pragma unroll
        for (int i = 0; i < QUILT_STAGE_UNROLL; ++i) {
            const int t = min(t0 + i * 256, n - 1);
            const int fy = t / fw, fx = t - fy * fw;
            uint32_t px[3];
            quilt_render3<SRC, LINEAR>(s, g, v, fx0 + fx, fy0 + fy, px);
            r[i] = px[0] | (px[1] << 8) | (px[2] << 16);
        }
#pragma unroll
        for (int i = 0; i < QUILT_STAGE_UNROLL; ++i)
            if (t0 + i * 256 < n) pix[t0 + i * 256] = r[i];
    }
}
// the same choice of source for one pixel (stm_k_quilt_area_px)
template <int SRC, bool LINEAR>
__device__ __forceinline__ void quilt_render3_any(const QuiltSrc &s, const QuiltGeom &g, int v, int x, int y, uint32_t (&px)[3])
{
    if constexpr (SRC == QSRC_SYNTH) {
        if (v == 0 || v == g.N - 1) { // view 0 = the right image, view N - 1 = the left image (d_io.cu:182-183)
            QuiltSrc e = s;
            e.image = v == 0 ? s.a.img_r : s.a.img_l;
            quilt_render3<QSRC_IMAGE, LINEAR>(e, g, v, x, y, px);
            return;
        }
    }
    quilt_render3<SRC, LINEAR>(s, g, v, x, y, px);
}

// Filter 1, the area average.  A workgroup owns bw x bh output pixels of tile blockIdx.z.  It renders every view pixel of the block's
// footprint once into LDS (three channels in one dword, from one load of the pixel's maps), reduces each footprint row with the
// column weights into 32-bit partial sums (at most 255 Win), then the partial sums with the row weights, rounds and writes u8.
// Integer arithmetic throughout, so the order of the sums does not matter.  LDS: [fh_max][fw_max] pixels, then [fh_max][BW][3] sums.
template <int SRC, bool LINEAR>
__global__ __launch_bounds__(256) void stm_k_quilt_area(QuiltSrc s, u8 *__restrict__ out, QuiltGeom g, int BW, int BH, int fw_max, int fh_max)
{
    extern __shared__ uint32_t quilt_lds[];
    if constexpr (SRC == QSRC_DEPTH)
        if (s.state) {
            s.gain = s.state[1];
            s.conv = s.state[2];
        }
    uint32_t *pix = quilt_lds, *hs = quilt_lds + (size_t)fw_max * fh_max;
    const int k = blockIdx.z;
    const int v = (g.order & 2) ? g.N - 1 - k : k;
    int left, top;
    quilt_tile_origin(g, k, left, top);
    const int u0 = blockIdx.x * BW, w0 = blockIdx.y * BH;
    const int bw = min(BW, g.tw - u0), bh = min(BH, g.th - w0);
    const int fx0 = (u0 * g.Win) / g.tw, fy0 = (w0 * g.Hin) / g.th;
    const int fw = ((u0 + bw) * g.Win - 1) / g.tw - fx0 + 1, fh = ((w0 + bh) * g.Hin - 1) / g.th - fy0 + 1; // <= fw_max, fh_max
    bool staged = false;
    if constexpr (SRC == QSRC_SYNTH)
        if (v == 0 || v == g.N - 1) { // view 0 = the right image, view N - 1 = the left image (d_io.cu:182-183): block-uniform
            s.image = v == 0 ? s.a.img_r : s.a.img_l;
            quilt_stage<QSRC_IMAGE, LINEAR>(s, g, v, fx0, fy0, fw, fh, pix);
            staged = true;
        }
    if (!staged) quilt_stage<SRC, LINEAR>(s, g, v, fx0, fy0, fw, fh, pix);
    __syncthreads();
    for (int t = threadIdx.x; t < fh * bw; t += 256) {
        const int fy = t / bw, u = u0 + (t - fy * bw);
        const int xa = (u * g.Win) / g.tw, xb = ((u + 1) * g.Win - 1) / g.tw;
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        const uint32_t *row = pix + fy * fw;
        for (int x = xa; x <= xb; ++x) {
            const uint32_t wx = quilt_weight(u, x, g.Win, g.tw), p = row[x - fx0];
            s0 += wx * (p & 255u);
            s1 += wx * ((p >> 8) & 255u);
            s2 += wx * (p >> 16);
        }
        hs[3 * t] = s0; hs[3 * t + 1] = s1; hs[3 * t + 2] = s2;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < bh * bw; t += 256) {
        const int wl = t / bw, ul = t - wl * bw;
        const int w = w0 + wl;
        const int ya = (w * g.Hin) / g.th, yb = ((w + 1) * g.Hin - 1) / g.th;
        unsigned long long a0 = 0, a1 = 0, a2 = 0;
        for (int y = ya; y <= yb; ++y) {
            const unsigned long long wy = quilt_weight(w, y, g.Hin, g.th);
            const uint32_t *h = hs + 3 * ((y - fy0) * bw + ul);
            a0 += wy * h[0];
            a1 += wy * h[1];
            a2 += wy * h[2];
        }
        u8 *o = out + ((size_t)(left + u0 + ul) + (size_t)(top + w) * g.Wout) * g.elem_sz;
        o[0] = quilt_round(a0, g); o[1] = quilt_round(a1, g); o[2] = quilt_round(a2, g);
    }
}
// The same average with one thread per output pixel looping over its own footprint: taken where even a 1 x 1 block's footprint
// does not fit the staging (a tiny tile of a large view).  Every view pixel is rendered by each output pixel that overlaps it.
template <int SRC, bool LINEAR>
__global__ __launch_bounds__(256) void stm_k_quilt_area_px(QuiltSrc s, u8 *__restrict__ out, QuiltGeom g)
{
    const int u = blockIdx.x * 256 + threadIdx.x, w = blockIdx.y, k = blockIdx.z;
    if (u >= g.tw) return;
    if constexpr (SRC == QSRC_DEPTH)
        if (s.state) {
            s.gain = s.state[1];
            s.conv = s.state[2];
        }
    const int v = (g.order & 2) ? g.N - 1 - k : k;
    int left, top;
    quilt_tile_origin(g, k, left, top);
    const int xa = (u * g.Win) / g.tw, xb = ((u + 1) * g.Win - 1) / g.tw;
    const int ya = (w * g.Hin) / g.th, yb = ((w + 1) * g.Hin - 1) / g.th;
    unsigned long long a0 = 0, a1 = 0, a2 = 0;
    for (int y = ya; y <= yb; ++y) {
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        for (int x = xa; x <= xb; ++x) {
            const uint32_t wx = quilt_weight(u, x, g.Win, g.tw);
            uint32_t px[3];
            quilt_render3_any<SRC, LINEAR>(s, g, v, x, y, px);
            s0 += wx * px[0];
            s1 += wx * px[1];
            s2 += wx * px[2];
        }
        const unsigned long long wy = quilt_weight(w, y, g.Hin, g.th);
        a0 += wy * s0;
        a1 += wy * s1;
        a2 += wy * s2;
    }
    u8 *o = out + ((size_t)(left + u) + (size_t)(top + w) * g.Wout) * g.elem_sz;
    o[0] = quilt_round(a0, g); o[1] = quilt_round(a1, g); o[2] = quilt_round(a2, g);
}

// ------------------------------------------------------------------ NV12 output (stm_hip.h, stm_set_output / stm_mux_nv12)
// The quilt's pixels converted where they are rendered: a thread (filter 0: four lanes) owns whole 2 x 2 blocks, renders their four
// pixels by the rules above (the rounded u8 values, as a BGR quilt would store them), and writes four Y samples and the block's
// U, V pair.  Every tile and both remainders are even (the frame call's screen), so a block lies in one tile or in none.
// The three functions below are the bodies of stm_k_quilt_nb, stm_k_quilt_area and stm_k_quilt_area_px, line for line, with the
// pixel handed back instead of stored: the BGR kernels above keep their own text, so their code is what it was.
// Filter 0: the three channels of output pixel (tx, ty) of tile (i, j) -- stm_k_mux's sampling position with the tile's size in place
// of the frame's, the four-neighbour sampler on the renderer's samples
template <int SRC, bool LINEAR>
__device__ __forceinline__ void quilt_nb_sample(const QuiltSrc &s, const QuiltGeom &g, int i, int j, int tx, int ty, u8 (&o)[3])
{
    const int k = j * g.tiles_x + i;
    const int v = (g.order & 2) ? g.N - 1 - k : k;
    int left, top;
    quilt_tile_origin(g, k, left, top);
    const int u = tx - left, w = ty - top;
    float xs = ((float)u / (float)g.tw) * (float)g.Win;
    xs = fminf(fmaxf(xs, 0.0f), (float)(g.Win - 1));
    float ys = ((float)w / (float)g.th) * (float)g.Hin;
    ys = fminf(fmaxf(ys, 0.0f), (float)(g.Hin - 1));
    if constexpr (SRC == QSRC_VIEWS) {
        const u8 *vw = s.views[v];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = bilinear_u8(vw, g.elem_sz, c, xs, ys, g.Win, g.Hin);
    } else {
        const int y0 = (int)floorf(ys);
        const int y1 = min(y0 + 1, g.Hin - 1);
        const float wy = ys - (float)y0;
        if constexpr (SRC == QSRC_SYNTH) {
            const int x0 = (int)floorf(xs);
            const int x1 = min(x0 + 1, g.Win - 1);
            const float wx = xs - (float)x0;
            const LensNb n00 = lens_nb(s.a, x0, y0, g.Win);
            LensNb n01 = n00, n10 = n00, n11 = n00; // only read where the weight is not 0
            if (wx != 0.0f) n01 = lens_nb(s.a, x1, y0, g.Win);
            if (wy != 0.0f) {
                n10 = lens_nb(s.a, x0, y1, g.Win);
                if (wx != 0.0f) n11 = lens_nb(s.a, x1, y1, g.Win);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = lens_bilinear<LINEAR, false>(s.a, n00, n01, n10, n11, wx, wy, g.N, v, 0.0f, c, g.Win, g.elem_sz);
        } else {
            DepthNbs nb;
            nb.x0 = -1;
            nb.has_x1 = false;
            const float sh = view_shift(v, g.N);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = depth_sample<LINEAR>(s.a, nb, sh, xs, y0, y1, wy, s.gain, s.conv, c, g.Win, g.elem_sz);
        }
    }
}
// the tile of output pixel (tx, ty); false: the pixel belongs to no tile
__device__ __forceinline__ bool quilt_nb_tile(const QuiltGeom &g, int tx, int ty, int &i, int &j)
{
    i = tx / g.tw;
    const int r = (g.order & 1) ? g.Hout - 1 - ty : ty; // rows counted from the edge the tile rows start at
    j = r / g.th;
    return i < g.tiles_x && j < g.tiles_y;
}
// the workgroup's block after the staging and the first reduction: where it lies and its partial sums
struct QuiltAreaBlock {
    int left, top, u0, w0, bw, bh, fy0;
    const uint32_t *hs;
};
template <int SRC, bool LINEAR>
__device__ __forceinline__ QuiltAreaBlock quilt_area_rows(QuiltSrc &s, const QuiltGeom &g, int BW, int BH, int fw_max, int fh_max)
{
    extern __shared__ uint32_t quilt_lds[];
    if constexpr (SRC == QSRC_DEPTH)
        if (s.state) {
            s.gain = s.state[1];
            s.conv = s.state[2];
        }
    uint32_t *pix = quilt_lds, *hs = quilt_lds + (size_t)fw_max * fh_max;
    const int k = blockIdx.z;
    const int v = (g.order & 2) ? g.N - 1 - k : k;
    int left, top;
    quilt_tile_origin(g, k, left, top);
    const int u0 = blockIdx.x * BW, w0 = blockIdx.y * BH;
    const int bw = min(BW, g.tw - u0), bh = min(BH, g.th - w0);
    const int fx0 = (u0 * g.Win) / g.tw, fy0 = (w0 * g.Hin) / g.th;
    const int fw = ((u0 + bw) * g.Win - 1) / g.tw - fx0 + 1, fh = ((w0 + bh) * g.Hin - 1) / g.th - fy0 + 1; // <= fw_max, fh_max
    bool staged = false;
    if constexpr (SRC == QSRC_SYNTH)
        if (v == 0 || v == g.N - 1) { // view 0 = the right image, view N - 1 = the left image (d_io.cu:182-183): block-uniform
            s.image = v == 0 ? s.a.img_r : s.a.img_l;
            quilt_stage<QSRC_IMAGE, LINEAR>(s, g, v, fx0, fy0, fw, fh, pix);
            staged = true;
        }
    if (!staged) quilt_stage<SRC, LINEAR>(s, g, v, fx0, fy0, fw, fh, pix);
    __syncthreads();
    for (int t = threadIdx.x; t < fh * bw; t += 256) {
        const int fy = t / bw, u = u0 + (t - fy * bw);
        const int xa = (u * g.Win) / g.tw, xb = ((u + 1) * g.Win - 1) / g.tw;
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        const uint32_t *row = pix + fy * fw;
        for (int x = xa; x <= xb; ++x) {
            const uint32_t wx = quilt_weight(u, x, g.Win, g.tw), p = row[x - fx0];
            s0 += wx * (p & 255u);
            s1 += wx * ((p >> 8) & 255u);
            s2 += wx * (p >> 16);
        }
        hs[3 * t] = s0; hs[3 * t + 1] = s1; hs[3 * t + 2] = s2;
    }
    __syncthreads();
    return QuiltAreaBlock{left, top, u0, w0, bw, bh, fy0, hs};
}
// the second reduction of the block's pixel (ul, wl), rounded
__device__ __forceinline__ void quilt_area_pixel(const QuiltAreaBlock &b, const QuiltGeom &g, int ul, int wl, u8 (&o)[3])
{
    const int w = b.w0 + wl;
    const int ya = (w * g.Hin) / g.th, yb = ((w + 1) * g.Hin - 1) / g.th;
    unsigned long long a0 = 0, a1 = 0, a2 = 0;
    for (int y = ya; y <= yb; ++y) {
        const unsigned long long wy = quilt_weight(w, y, g.Hin, g.th);
        const uint32_t *h = b.hs + 3 * ((y - b.fy0) * b.bw + ul);
        a0 += wy * h[0];
        a1 += wy * h[1];
        a2 += wy * h[2];
    }
    o[0] = quilt_round(a0, g); o[1] = quilt_round(a1, g); o[2] = quilt_round(a2, g);
}
// The same average of tile pixel (u, w) of view v by one thread looping over the pixel's own footprint: every view pixel is rendered
// by each output pixel that overlaps it
template <int SRC, bool LINEAR>
__device__ __forceinline__ void quilt_area_own(const QuiltSrc &s, const QuiltGeom &g, int v, int u, int w, u8 (&o)[3])
{
    const int xa = (u * g.Win) / g.tw, xb = ((u + 1) * g.Win - 1) / g.tw;
    const int ya = (w * g.Hin) / g.th, yb = ((w + 1) * g.Hin - 1) / g.th;
    unsigned long long a0 = 0, a1 = 0, a2 = 0;
    for (int y = ya; y <= yb; ++y) {
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        for (int x = xa; x <= xb; ++x) {
            const uint32_t wx = quilt_weight(u, x, g.Win, g.tw);
            uint32_t px[3];
            quilt_render3_any<SRC, LINEAR>(s, g, v, x, y, px);
            s0 += wx * px[0];
            s1 += wx * px[1];
            s2 += wx * px[2];
        }
        const unsigned long long wy = quilt_weight(w, y, g.Hin, g.th);
        a0 += wy * s0;
        a1 += wy * s1;
        a2 += wy * s2;
    }
    o[0] = quilt_round(a0, g); o[1] = quilt_round(a1, g); o[2] = quilt_round(a2, g);
}
// A block's two samples of a plane row leave as one 16-bit store where both planes' bases and pitches are even, as bytes otherwise.
__device__ __forceinline__ void nv12_store_pair(u8 *p, uint32_t a, uint32_t b, int pairs)
{
    if (pairs) {
        *(unsigned short *)p = (unsigned short)(a | (b << 8));
    } else {
        p[0] = (u8)a;
        p[1] = (u8)b;
    }
}
__device__ __forceinline__ int nv12_luma(const Nv12OutCoef &k, int b, int g, int r)
{
    return (k.yr * r + k.yg * g + k.yb * b + (k.yo << 16) + 32768) >> 16; // in 0 .. 255 for every pixel: no clip
}
// U and V of a block from the sums of its four pixels' B, G and R
__device__ __forceinline__ void nv12_chroma(const Nv12OutCoef &k, int sb, int sg, int sr, int &U, int &V)
{
    U = min(max((k.h * sb - k.ug * sg - k.ur * sr + (128 << 18) + (1 << 17)) >> 18, 0), 255);
    V = min(max((k.h * sr - k.vg * sg - k.vb * sb + (128 << 18) + (1 << 17)) >> 18, 0), 255);
}
// stm_mux_nv12's arithmetic on the block at even (x, y): px = its pixels (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1) as B, G, R
__device__ __forceinline__ void nv12_store_block(const Nv12Out &o, int x, int y, const u8 (&px)[4][3])
{
    const Nv12OutCoef &k = o.k;
    int Y[4], sb = 0, sg = 0, sr = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int b = px[q][0], gr = px[q][1], r = px[q][2];
        Y[q] = nv12_luma(k, b, gr, r);
        sb += b;
        sg += gr;
        sr += r;
    }
    int U, V;
    nv12_chroma(k, sb, sg, sr, U, V);
    u8 *py = o.y + (size_t)y * o.pitch_y + x;
    nv12_store_pair(py, Y[0], Y[1], o.pairs);
    nv12_store_pair(py + o.pitch_y, Y[2], Y[3], o.pairs);
    nv12_store_pair(o.uv + (size_t)(y >> 1) * o.pitch_uv + x, U, V, o.pairs);
}

// The conversion as a stage (stm_mux_nv12), and the un-fused frame's second kernel: one thread per 2 x 2 block of img
__global__ __launch_bounds__(256) void stm_k_mux_nv12(Nv12Out o, const u8 *__restrict__ img, int W, int elem_sz)
{
    const int x = 2 * (blockIdx.x * 256 + threadIdx.x), y = 2 * blockIdx.y;
    if (x >= W) return;
    u8 px[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const u8 *p = img + ((size_t)(y + (q >> 1)) * W + x + (q & 1)) * elem_sz;
        px[q][0] = p[0]; px[q][1] = p[1]; px[q][2] = p[2];
    }
    nv12_store_block(o, x, y, px);
}
void launch_mux_nv12(const Nv12Out &o, const u8 *img, int H, int W, int elem_sz)
{
    ProfScope p("mux_nv12");
    STM_LAUNCH(stm_k_mux_nv12, dim3(cdiv(W / 2, 256), H / 2), dim3(256), 0, stream(), o, img, W, elem_sz);
    STM_CHECK_LAUNCH();
}

// Filter 0 into NV12: four adjacent lanes own a 2 x 2 block, one pixel each, rendered as stm_k_quilt_nb renders it -- a wave has the
// loads of 64 pixels in flight, as there; one thread rendering the block's four pixels in turn took 2.4 times as long (DESIGN.md
// section 20).  A row's neighbour and the block's sums cross the lanes; a block of no tile is (0, 0, 0) four times.
template <int SRC, bool LINEAR>
__global__ __launch_bounds__(256) void stm_k_quilt_nb_nv12(QuiltSrc s, Nv12Out o, QuiltGeom g)
{
    const int t = blockIdx.x * 256 + threadIdx.x, sub = t & 3;
    const int bx = 2 * (t >> 2), by = 2 * blockIdx.y;
    if (bx >= g.Wout) return; // the four lanes of a block leave together
    if constexpr (SRC == QSRC_DEPTH)
        if (s.state) {
            s.gain = s.state[1];
            s.conv = s.state[2];
        }
    const int tx = bx + (sub & 1), ty = by + (sub >> 1);
    u8 px[3] = {0, 0, 0};
    int i, j;
    if (quilt_nb_tile(g, tx, ty, i, j)) quilt_nb_sample<SRC, LINEAR>(s, g, i, j, tx, ty, px); // the same for all four lanes
    const uint32_t Y = (uint32_t)nv12_luma(o.k, px[0], px[1], px[2]);
    const uint32_t Yn = (uint32_t)__shfl_xor((int)Y, 1);
    uint32_t sum = px[0] | ((uint32_t)px[1] << 10) | ((uint32_t)px[2] << 20); // three sums of at most 1020, ten bits each
    sum += (uint32_t)__shfl_xor((int)sum, 1);
    sum += (uint32_t)__shfl_xor((int)sum, 2);
    u8 *py = o.y + (size_t)ty * o.pitch_y + tx;
    if (!o.pairs) *py = (u8)Y;
    else if (!(sub & 1)) *(unsigned short *)py = (unsigned short)(Y | (Yn << 8));
    if (sub == 0) {
        int U, V;
        nv12_chroma(o.k, sum & 1023u, (sum >> 10) & 1023u, sum >> 20, U, V);
        nv12_store_pair(o.uv + (size_t)(by >> 1) * o.pitch_uv + bx, U, V, o.pairs);
    }
}
// Filter 1 into NV12: stm_k_quilt_area with its last phase walking the 2 x 2 blocks of the workgroup's pixels (BW and BH even)
template <int SRC, bool LINEAR>
__global__ __launch_bounds__(256) void stm_k_quilt_area_nv12(QuiltSrc s, Nv12Out o, QuiltGeom g, int BW, int BH, int fw_max, int fh_max)
{
    const QuiltAreaBlock b = quilt_area_rows<SRC, LINEAR>(s, g, BW, BH, fw_max, fh_max);
    const int cw = b.bw >> 1;
    for (int t = threadIdx.x; t < (b.bh >> 1) * cw; t += 256) {
        const int wl = 2 * (t / cw), ul = 2 * (t % cw);
        u8 px[4][3];
#pragma unroll
        for (int q = 0; q < 4; ++q) quilt_area_pixel(b, g, ul + (q & 1), wl + (q >> 1), px[q]);
        nv12_store_block(o, b.left + b.u0 + ul, b.top + b.w0 + wl, px);
    }
}
// ... and the per-pixel form with one thread per 2 x 2 block, where not even such a block's footprint fits the staging
template <int SRC, bool LINEAR>
__global__ __launch_bounds__(256) void stm_k_quilt_area_px_nv12(QuiltSrc s, Nv12Out o, QuiltGeom g)
{
    const int u = 2 * (blockIdx.x * 256 + threadIdx.x), w = 2 * blockIdx.y, k = blockIdx.z;
    if (u >= g.tw) return;
    if constexpr (SRC == QSRC_DEPTH)
        if (s.state) {
            s.gain = s.state[1];
            s.conv = s.state[2];
        }
    const int v = (g.order & 2) ? g.N - 1 - k : k;
    int left, top;
    quilt_tile_origin(g, k, left, top);
    u8 px[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) quilt_area_own<SRC, LINEAR>(s, g, v, u + (q & 1), w + (q >> 1), px[q]);
    nv12_store_block(o, left + u, top + w, px);
}
// the blocks of no tile (stm_k_quilt_pad's pixels, both remainders even): Y of black and 128 / 128
__global__ __launch_bounds__(256) void stm_k_quilt_pad_nv12(Nv12Out o, QuiltGeom g, int rem_w, int rem_h)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t bw = (size_t)(rem_w >> 1), n_right = bw * (g.Hout >> 1), used_w = (size_t)((g.Wout - rem_w) >> 1);
    int x, y;
    if (t < n_right) {
        y = (int)(t / bw);
        x = (int)used_w + (int)(t - (size_t)y * bw);
    } else {
        const size_t q = t - n_right;
        if (q >= used_w * (rem_h >> 1)) return;
        const int r = (int)(q / used_w);
        x = (int)(q - (size_t)r * used_w);
        y = (g.order & 1) ? r : ((g.Hout - rem_h) >> 1) + r; // bottom-up tiles leave the top rows
    }
    const u8 px[4][3] = {};
    nv12_store_block(o, 2 * x, 2 * y, px);
}

// The block of the staged kernel: the largest of 32 x 16, halved along the axis with the longer footprint, whose staging fits
// `limit` bytes of LDS; false where not even one output pixel's footprint does.  least = 2 (NV12): BW and BH stay even, and false where
// not even a 2 x 2 block's footprint fits.
static bool quilt_block(const QuiltGeom &g, size_t limit, int &BW, int &BH, int &fw_max, int &fh_max, size_t &bytes, int least = 1)
{
    BW = 32;
    BH = 16;
    for (;;) {
        fw_max = min(g.Win, cdiv(BW * g.Win, g.tw) + 1); // tw Win and th Hin fit an int (quilt_args_ok)
        fh_max = min(g.Hin, cdiv(BH * g.Hin, g.th) + 1);
        bytes = 4 * ((size_t)fw_max * fh_max + (size_t)fh_max * BW * 3);
        if (bytes <= limit) return true;
        if (BH > least && (fh_max >= fw_max || BW == least)) BH /= 2;
        else if (BW > least) BW /= 2;
        else return false;
    }
}
// the same pixels into an NV12 surface: every kernel's NV12 form, a thread per 2 x 2 block
template <int SRC, bool LINEAR>
static void launch_quilt_src_nv12(const QuiltSrc &s, const Nv12Out &o, const QuiltGeom &g, int filter)
{
    if (filter == 0) {
        STM_LAUNCH((stm_k_quilt_nb_nv12<SRC, LINEAR>), dim3(cdiv(2 * g.Wout, 256), g.Hout / 2), dim3(256), 0, stream(), s, o, g);
        return;
    }
    const int rem_w = g.Wout - g.tiles_x * g.tw, rem_h = g.Hout - g.tiles_y * g.th;
    const size_t n_pad = ((size_t)rem_w * g.Hout + (size_t)(g.Wout - rem_w) * rem_h) / 4;
    if (n_pad) STM_LAUNCH(stm_k_quilt_pad_nv12, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, stream(), o, g, rem_w, rem_h);
    int BW, BH, fw_max, fh_max;
    size_t bytes;
    if (quilt_block(g, (size_t)quilt_lds_limit(), BW, BH, fw_max, fh_max, bytes, 2))
        STM_LAUNCH((stm_k_quilt_area_nv12<SRC, LINEAR>), dim3(cdiv(g.tw, BW), cdiv(g.th, BH), g.N), dim3(256), bytes, stream(), s, o, g, BW, BH,
                   fw_max, fh_max);
    else
        STM_LAUNCH((stm_k_quilt_area_px_nv12<SRC, LINEAR>), dim3(cdiv(g.tw / 2, 256), g.th / 2, g.N), dim3(256), 0, stream(), s, o, g);
}
template <int SRC, bool LINEAR>
static void launch_quilt_src(const QuiltSrc &s, u8 *out, const QuiltGeom &g, int filter, const Nv12Out *nv = nullptr)
{
    if constexpr (SRC != QSRC_VIEWS) // a table of views is never tiled into NV12: the un-fused frame converts its BGR quilt
        if (nv) {
            launch_quilt_src_nv12<SRC, LINEAR>(s, *nv, g, filter);
            return;
        }
    const dim3 full(cdiv(g.Wout, 256), g.Hout);
    if (filter == 0) {
        STM_LAUNCH((stm_k_quilt_nb<SRC, LINEAR>), full, dim3(256), 0, stream(), s, out, g);
        return;
    }
    const int rem_w = g.Wout - g.tiles_x * g.tw, rem_h = g.Hout - g.tiles_y * g.th;
    const size_t n_pad = (size_t)rem_w * g.Hout + (size_t)(g.Wout - rem_w) * rem_h;
    if (n_pad) STM_LAUNCH(stm_k_quilt_pad, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, stream(), out, g, rem_w, rem_h);
    int BW, BH, fw_max, fh_max;
    size_t bytes;
    if (quilt_block(g, (size_t)quilt_lds_limit(), BW, BH, fw_max, fh_max, bytes))
        STM_LAUNCH((stm_k_quilt_area<SRC, LINEAR>), dim3(cdiv(g.tw, BW), cdiv(g.th, BH), g.N), dim3(256), bytes, stream(), s, out, g, BW, BH,
                   fw_max, fh_max);
    else
        STM_LAUNCH((stm_k_quilt_area_px<SRC, LINEAR>), dim3(cdiv(g.tw, 256), g.th, g.N), dim3(256), 0, stream(), s, out, g);
}
static QuiltGeom quilt_geom(const Layout &lo, int N, int Hin, int Win, int Hout, int Wout, int elem_sz)
{
    QuiltGeom g{N, lo.tiles_x, lo.tiles_y, lo.order, Wout / lo.tiles_x, Hout / lo.tiles_y, Hin, Win, Hout, Wout, elem_sz, 0};
    const unsigned long long den = (unsigned long long)Win * (unsigned long long)Hin;
    g.narrow = 255ull * den + den / 2 <= 0xffffffffull;
    return g;
}
// lo screened by the caller (quilt_args_ok)
void launch_quilt(const u8 *const *d_views, u8 *out, int N, const Layout &lo, int Hin, int Win, int Hout, int Wout, int elem_sz)
{
    QuiltSrc s{};
    s.views = d_views;
    ProfScope p("quilt");
    launch_quilt_src<QSRC_VIEWS, false>(s, out, quilt_geom(lo, N, Hin, Win, Hout, Wout, elem_sz), lo.filter);
    STM_CHECK_LAUNCH();
}
// depth_mode 0: synth_sample's views; 1, 2: the depth budget's (state != nullptr: gain and conv are read on the device)
void launch_synth_quilt(const u8 *img_l, const u8 *img_r, const float *disp_l, const float *disp_r, const float *mask_l, const float *mask_r,
                        const float *blend, u8 *out, int N, const Layout &lo, int depth_mode, float gain, float conv, const float *state,
                        int Hin, int Win, int Hout, int Wout, int elem_sz, bool linear, const Nv12Out *nv)
{
    QuiltSrc s{};
    s.a = SynthArgs{img_l, img_r, disp_l, disp_r, mask_l, mask_r, blend};
    s.gain = gain;
    s.conv = conv;
    s.state = state;
    const QuiltGeom g = quilt_geom(lo, N, Hin, Win, Hout, Wout, elem_sz);
    ProfScope p("synth_quilt");
    if (depth_mode == 0) {
        if (linear) launch_quilt_src<QSRC_SYNTH, true>(s, out, g, lo.filter, nv);
        else launch_quilt_src<QSRC_SYNTH, false>(s, out, g, lo.filter, nv);
    } else {
        if (linear) launch_quilt_src<QSRC_DEPTH, true>(s, out, g, lo.filter, nv);
        else launch_quilt_src<QSRC_DEPTH, false>(s, out, g, lo.filter, nv);
    }
    STM_CHECK_LAUNCH();
}

} // namespace stm
