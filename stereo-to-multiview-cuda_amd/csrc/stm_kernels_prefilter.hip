// stm_kernels_prefilter.hip -- view antialiasing: the depth-adaptive horizontal prefilter of the two images the views are rendered
// from (stm_view_prefilter, stm_set_antialias; include/stm_hip.h has the definition line by line, DESIGN.md section 22 the reasons).
//
// A workgroup of 256 lanes owns 256 consecutive pixels of one row of one image.  It stages them and a 16-pixel halo on either side
// in LDS -- a pixel as one dword B | G << 8 | R << 16, its delta as f32 -- so global memory is read once and every tap comes from
// LDS; the halo repeats the row's end pixels, which is the definition's clamp.  One lane, one pixel.  A wave none of whose pixels
// has H != 0 stores what it loaded (on most frames most waves); the others walk k = 1 .. K, each lane to its own K <= 16.
//
// The quotient.  n = 16 c + sum + (T >> 1) <= 255 * 528 + 264 and T in 16 .. 528 are integers below 2^24, exact as f32.  The f32
// division is correctly rounded (this file is built without fast-math, and hipcc's default keeps `/` correctly rounded).  If T
// divides n the quotient is an integer below 2^24 and comes out exact.  Otherwise n / T lies at least 1 / T >= 1 / 528 below the next
// integer, while rounding moves it by at most 2^-24 * 256 -- it cannot reach that integer, and truncation gives floor(n / T).
#include "stm_common.h"
#include <float.h>

namespace stm {

namespace {
constexpr int PF_SEG = 256, PF_HALO = 16; // K <= 16 because max_radius <= 16

struct PrefilterArgs {
    const u8 *in[2];
    u8 *out[2];
    const float *disp[2];
    int W, elem_sz;
    float k16, hmax, gate, gain, conv;
    const float *state; // depth mode 2: gain and conv are read from state[1], state[2]
};

__device__ __forceinline__ uint32_t pf_load_bytes(const u8 *s) { return (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16); }
} // namespace

__global__ __launch_bounds__(PF_SEG) void stm_k_view_prefilter(PrefilterArgs a)
{
    __shared__ uint32_t s_px[PF_SEG + 2 * PF_HALO];
    __shared__ float s_dl[PF_SEG + 2 * PF_HALO];
    const int tid = threadIdx.x, lane = tid & 63, y = blockIdx.y, v = blockIdx.z, W = a.W, E = a.elem_sz;
    const int seg0 = blockIdx.x * PF_SEG, w0 = seg0 + (tid & ~63); // the wave's first pixel
    const int x = seg0 + tid, xc = min(x, W - 1);
    const u8 *__restrict__ in = a.in[v] + (size_t)y * W * E;
    u8 *__restrict__ out = a.out[v] + (size_t)y * W * E;
    const float *__restrict__ dl = a.disp[v] + (size_t)y * W;
    // Every lane loads, also one past the row's end (xc): a tap of a pixel x < W at x + k >= W must see pixel W - 1, so the whole
    // tile is filled with clamped loads.  The wave's 64 pixels go as whole dwords where the row segment allows it (stm_k_front's
    // store phase): 3-byte pixels are 48 aligned dwords, each lane's pixel built from two of them; 4-byte pixels are one dword
    // each on the way in.  Otherwise byte by byte, any alignment.
    const bool full = w0 + 64 <= W;
    const bool in3 = E == 3 && full && (((uintptr_t)(in + (size_t)w0 * 3)) & 3) == 0;
    const bool out3 = E == 3 && full && (((uintptr_t)(out + (size_t)w0 * 3)) & 3) == 0;
    const bool in4 = E == 4 && (((uintptr_t)in) & 3) == 0;
    uint32_t px;
    if (in3) {
        const uint32_t dw = ((const uint32_t *)(in + (size_t)w0 * 3))[min(lane, 47)];
        const int d0 = (3 * lane) >> 2, sh = 8 * ((3 * lane) & 3);
        const uint32_t lo = (uint32_t)__shfl((int)dw, d0), hi = (uint32_t)__shfl((int)dw, min(d0 + 1, 47));
        px = (uint32_t)((lo | ((unsigned long long)hi << 32)) >> sh) & 0xffffffu;
    } else if (in4) {
        px = ((const uint32_t *)in)[xc] & 0xffffffu;
    } else {
        px = pf_load_bytes(in + (size_t)xc * E);
    }
    const float d = dl[xc];
    s_px[tid + PF_HALO] = px;
    s_dl[tid + PF_HALO] = d;
    if (tid < 2 * PF_HALO) { // the halo: 16 pixels left of the segment, 16 right of it, clamped to the row
        const int pos = tid < PF_HALO ? tid : PF_SEG + tid;
        const int gx = min(max(seg0 - PF_HALO + pos, 0), W - 1);
        s_px[pos] = pf_load_bytes(in + (size_t)gx * E);
        s_dl[pos] = dl[gx];
    }
    float gain = a.gain, conv = a.conv;
    if (a.state) { // automatic depth mode: what stm_k_depth_fit left for this frame
        gain = a.state[1];
        conv = a.state[2];
    }
    // the per-side extension in 1/16 px (stm_hip.h): one rounding per line
    const float p = __fmul_rn(gain, d);
    const float e = __fsub_rn(p, conv);
    const float ab = fabsf(e);
    int Hx = 0;
    if (ab <= FLT_MAX) Hx = (int)__fadd_rn(fminf(__fmul_rn(ab, a.k16), a.hmax), 0.5f); // (false for NaN and inf)
    __syncthreads();
    uint32_t o = px;
    if (__ballot(Hx != 0) != 0ull) {
        const int K = (Hx + 15) >> 4;
        uint32_t sb = 0, sg = 0, sr = 0, T = 16;
        for (int k = 1; k <= K; ++k) {
            const uint32_t wk = (uint32_t)min(16, Hx - 16 * (k - 1));
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const int q = tid + PF_HALO + (side ? k : -k);
                const bool used = fabsf(__fsub_rn(s_dl[q], d)) <= a.gate; // (false for NaN)
                const uint32_t t = s_px[q], w = used ? wk : 0u;
                sb += w * (t & 0xffu);
                sg += w * ((t >> 8) & 0xffu);
                sr += w * (t >> 16);
                T += w;
            }
        }
        const float Tf = (float)T;
        const uint32_t half = T >> 1;
        const uint32_t ob = (uint32_t)((float)(16u * (px & 0xffu) + sb + half) / Tf);
        const uint32_t og = (uint32_t)((float)(16u * ((px >> 8) & 0xffu) + sg + half) / Tf);
        const uint32_t orr = (uint32_t)((float)(16u * (px >> 16) + sr + half) / Tf);
        o = ob | (og << 8) | (orr << 16);
    }
    if (out3) {
        const int p0 = (4 * lane) / 3, o8 = 8 * (4 * lane - 3 * p0); // lane < 48: dword `lane` starts in byte o8 / 8 of pixel p0
        const uint32_t lo = (uint32_t)__shfl((int)o, p0 & 63), hi = (uint32_t)__shfl((int)o, (p0 + 1) & 63);
        if (lane < 48) ((uint32_t *)(out + (size_t)w0 * 3))[lane] = (uint32_t)((lo | ((unsigned long long)hi << 24)) >> o8);
    } else if (x < W) {
        u8 *q = out + (size_t)x * E; // bytes past the third are left alone
        q[0] = (u8)o; q[1] = (u8)(o >> 8); q[2] = (u8)(o >> 16);
    }
}

// one launch for nimg (1 or 2) images, each filtered by its own map; state != nullptr: gain and conv are read on the device.
// Screened by the caller (stm_api.hip, prefilter_args_ok; the frame calls' own screens)
void launch_view_prefilter(int nimg, u8 *const *out, const u8 *const *in, const float *const *disp, int H, int W, int elem_sz, int num_views,
                           float strength, int max_radius, float gate, float gain, float conv, const float *state)
{
    PrefilterArgs a = {};
    for (int i = 0; i < nimg; ++i) { a.in[i] = in[i]; a.out[i] = out[i]; a.disp[i] = disp[i]; }
    a.W = W; a.elem_sz = elem_sz;
    a.k16 = (float)((double)strength * 8.0 / (double)(num_views - 1));
    a.hmax = (float)(16 * max_radius);
    a.gate = gate; a.gain = gain; a.conv = conv; a.state = state;
    ProfScope p("prefilter");
    STM_LAUNCH(stm_k_view_prefilter, dim3(cdiv(W, PF_SEG), H, nimg), dim3(PF_SEG), 0, stream(), a);
    STM_CHECK_LAUNCH();
}

} // namespace stm
