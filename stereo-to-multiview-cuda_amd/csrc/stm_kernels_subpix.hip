// stm_kernels_subpix.hip -- sub-pixel disparity enhancement (Mei et al. 3.4, last step): a parabola through the aggregated
// costs at d - 1, d, d + 1 moves a whole-pixel disparity by at most half a pixel.  An addition: the reference has no such step.
//
// Definition (include/stm_hip.h): v = disp[p] is eligible when it is a whole number with
// 1 <= v + zd <= D - 2 and the three costs cm = C[d-1][p], c0 = C[d][p], cp = C[d+1][p] are finite; then, in f32 and in this
// order, den = (cm + cp) - (c0 + c0), and if den > 0: out = v + clamp((cm - cp) / (den + den), -0.5, 0.5).  The build's
// -ffp-contract=off and correctly rounded division make that bit-identical to a numpy float32 statement of the same lines.
//
// Two kernels share subpix_refine():
//   stm_k_subpix_vol    the per-stage call: the materialised volume (plane table or slab), three loads per pixel.
//   stm_k_subpix_frame  the frame pipeline, where the aggregated volume is never written (its last horizontal pass is fused
//                       with WTA).  What is still in memory is that pass's input V2; the three needed costs are rebuilt from
//                       it exactly as the pass computes them: C[k][y][x] = sum of V2[k][y][x'], x' = x - armL .. x + armR - 1,
//                       ascending, from 0.0f (oracle/stm_oracle.c orc_agg_hpass).  One lane per pixel, lanes along x: the
//                       lanes of a wave walk overlapping windows, so a record fetched for one lane serves its neighbours
//                       from L1 / L2.  Both views in one launch; templated on the volume layout (PQ of the matrix-pipe
//                       kernels, quads of the vector-ALU kernels).
#include "stm_common.h"

namespace stm {

typedef float sp_f4 __attribute__((ext_vector_type(4)));

// the pixel's whole-pixel hypothesis d = v + zd, or -1 when v is not eligible (not a whole number, NaN, +-inf, or d outside
// 1 .. D - 2: a parabola needs both neighbours)
__device__ __forceinline__ int subpix_index(float v, int D, int zd)
{
    if (!(v == floorf(v))) return -1; // NaN, non-integer
    if (!(v >= (float)(1 - zd) && v <= (float)(D - 2 - zd))) return -1; // +-inf, out of range (small integers: exact in f32)
    return (int)v + zd;
}

// the enhancement of one eligible pixel; every line is one f32 operation (no contraction in this file's build)
__device__ __forceinline__ float subpix_refine(float v, float cm, float c0, float cp)
{
    if (!(isfinite(cm) && isfinite(c0) && isfinite(cp))) return v;
    const float s = cm + cp;
    const float t = c0 + c0;
    const float den = s - t;
    if (!(den > 0.0f)) return v; // flat or concave: no minimum between the neighbours
    const float num = cm - cp;
    const float den2 = den + den;
    float off = num / den2; // correctly rounded (no __fdividef / rcp)
    off = fminf(fmaxf(off, -0.5f), 0.5f); // a voted d need not be a local minimum of the cost
    return v + off;
}

// ------------------------------------------------------------------ per-stage: the materialised volume
__global__ __launch_bounds__(256) void stm_k_subpix_vol(Vol cost, float *__restrict__ disp, int D, int zd, size_t HW)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const float v = disp[p];
    const int d = subpix_index(v, D, zd);
    if (d < 0) return;
    disp[p] = subpix_refine(v, cost.plane(d - 1)[p], cost.plane(d)[p], cost.plane(d + 1)[p]);
}

void launch_subpix(Vol cost, float *disp, int D, int zd, int H, int W)
{
    const size_t HW = (size_t)H * W;
    ProfScope p("subpixel");
    STM_LAUNCH(stm_k_subpix_vol, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, stream(), cost, disp, D, zd, HW);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ frame pipeline: the three costs from V2
// Volume accessors: the four pixels 4g .. 4g+3 of hypothesis k in row y of one view.
// PQ (stm_kernels_aggm.hip): float4 [k / 16][y][g][k % 16], one 16-byte load; the hypotheses d - 1 .. d + 1 of a group sit
// in the same 256-byte record unless they straddle a chunk boundary.  Pixels >= W of the last group are padding (read,
// never summed).
struct SubpixPQ {
    const float *v[2];
    int H, G;
    __device__ __forceinline__ sp_f4 group(int view, int k, int y, int g, int) const
    {
        const sp_f4 *b = (const sp_f4 *)v[view];
        return b[(((size_t)(k >> 4) * H + y) * G + g) * 16 + (k & 15)];
    }
};
// QUADS (stm_common.h Vol::quad): float4 [k / 4][y][x], the four hypotheses of a pixel in one element; four dword loads, the
// columns beyond the image clamped to W - 1 (their values are never summed)
struct SubpixQuads {
    const float *v[2];
    size_t plane;
    __device__ __forceinline__ sp_f4 group(int view, int k, int y, int g, int W) const
    {
        const float *b = v[view] + ((size_t)(k >> 2) * plane + (size_t)y * W) * 4 + (k & 3);
        sp_f4 r;
        r.x = b[(size_t)min(4 * g, W - 1) * 4];
        r.y = b[(size_t)min(4 * g + 1, W - 1) * 4];
        r.z = b[(size_t)min(4 * g + 2, W - 1) * 4];
        r.w = b[(size_t)min(4 * g + 3, W - 1) * 4];
        return r;
    }
};

template <class ACC>
__global__ __launch_bounds__(256) void stm_k_subpix_frame(ACC acc, float *disp_a, const u8 *__restrict__ armL_a,
                                                          const u8 *__restrict__ armR_a, float *disp_b, const u8 *__restrict__ armL_b,
                                                          const u8 *__restrict__ armR_b, int D, int zd, int H, int W)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, view = blockIdx.z;
    if (x >= W) return;
    float *disp = view ? disp_b : disp_a;
    const size_t p = (size_t)y * W + x;
    const float v = disp[p];
    const int d = subpix_index(v, D, zd);
    if (d < 0) return;
    // the window [a, b) of the last horizontal pass; arms never reach past the image (x - armL >= 0, x + armR <= W - 1), the
    // clamps only keep the reads inside the volume whatever the arm planes hold
    const int a = max(x - (int)(view ? armL_b : armL_a)[p], 0), b = min(x + (int)(view ? armR_b : armR_a)[p], W);
    float sm = 0.0f, s0 = 0.0f, sp = 0.0f;
    if (a < b) {
        const int g1 = (b - 1) >> 2;
        for (int g = a >> 2; g <= g1; ++g) {
            const sp_f4 vm = acc.group(view, d - 1, y, g, W), v0 = acc.group(view, d, y, g, W), vp = acc.group(view, d + 1, y, g, W);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int xi = 4 * g + i;
                const bool in = xi >= a && xi < b; // ascending x', one rounding per element, nothing added outside the window
                sm = in ? sm + vm[i] : sm;
                s0 = in ? s0 + v0[i] : s0;
                sp = in ? sp + vp[i] : sp;
            }
        }
    }
    disp[p] = subpix_refine(v, sm, s0, sp);
}

// pq != nullptr: the PQ volumes V2 of the two views (launch_aggm_frame's vol_a); else quads[2] (the vector-ALU chain's
// inputs of launch_agg_h_wta2), plane stride H * W float4 elements.  disp[2] refined in place.
void launch_subpix_frame(float *const *pq, float *const *quads, float *const *disp, const u8 *const *armL, const u8 *const *armR, int D,
                         int zd, int H, int W)
{
    ProfScope p("subpixel");
    const dim3 grid(cdiv(W, 256), H, 2);
    if (pq) {
        SubpixPQ acc;
        acc.v[0] = pq[0]; acc.v[1] = pq[1]; acc.H = H; acc.G = (W + 3) / 4;
        STM_LAUNCH(stm_k_subpix_frame<SubpixPQ>, grid, dim3(256), 0, stream(), acc, disp[0], armL[0], armR[0], disp[1], armL[1],
                   armR[1], D, zd, H, W);
    } else {
        SubpixQuads acc;
        acc.v[0] = quads[0]; acc.v[1] = quads[1]; acc.plane = (size_t)H * W;
        STM_LAUNCH(stm_k_subpix_frame<SubpixQuads>, grid, dim3(256), 0, stream(), acc, disp[0], armL[0], armR[0], disp[1], armL[1],
                   armR[1], D, zd, H, W);
    }
    STM_CHECK_LAUNCH();
}

} // namespace stm
