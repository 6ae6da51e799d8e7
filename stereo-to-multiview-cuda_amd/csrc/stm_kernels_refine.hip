// stm_kernels_refine.hip -- disparity refinement for gfx950: L/R consistency check, iterative region
// voting, bilateral filter on the disparity map, grow-only gaussian.
//
// Reference stages replaced:
//   dr_dcc_kernel / dr_ddc_kernel / dr_merge_errors_kernel   d_dr_dcc.cu:57-82 / :35-54 / :18-33
//   dr_irv_pre_kernel / dr_irv_kernel_3                      d_dr_irv.cu:134-220 / :17-43
//   filter_bilateral_1_kernel_6                              d_filter_bilateral.cu:222-304
//   filter_gaussian_1_kernel_1 (+ op_invertnormf_kernel)     d_filter_gaussian.cu:9-88 (d_op.cu:7-16)
// All of them are image-sized (<= 17 B/px of HBM traffic) and LDS/latency bound; accumulation orders
// follow the reference loops exactly (row-major taps, sequential float adds, no contraction).
#include "stm_common.h"
#include <type_traits>
#include <mutex>

#include <map>
#include <utility>
#include <vector>

namespace stm {

// ------------------------------------------------------------------ L/R check
// phase 1: outlier flags + hit-map scatter (both scatters only ever write the value 0 -> benign races)
__global__ __launch_bounds__(256) void stm_k_dcc_mark(u8 *__restrict__ out_l, u8 *__restrict__ out_r,
                                                      const float *__restrict__ disp_l, const float *__restrict__ disp_r,
                                                      u8 *__restrict__ hit_l, u8 *__restrict__ hit_r, int H, int W)
{
    int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    size_t row = (size_t)y * W;
    const float thresh = 1.0f; // d_dr_dcc.cu:117
    float dl = disp_l[row + x];
    int c = map_col(x, (int)dl, W); // a caller's map: the conversion saturates, the sum must not wrap
    if (fabsf(dl - disp_r[row + c]) > thresh) out_l[row + x] = 1;
    hit_r[row + c] = 0; // dr_ddc_kernel: same coordinate (d_dr_dcc.cu:45-48)
    float dr = disp_r[row + x];
    c = map_col_sub(x, (int)dr, W);
    if (fabsf(dr - disp_l[row + c]) > thresh) out_r[row + x] = 1;
    hit_l[row + c] = 0;
}
// phase 2: outlier and never hit -> class 2 (occlusion)
__global__ __launch_bounds__(256) void stm_k_dcc_merge(u8 *__restrict__ out_l, u8 *__restrict__ out_r,
                                                       const u8 *__restrict__ hit_l, const u8 *__restrict__ hit_r, size_t HW)
{
    size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    if (out_l[p] == 1 && hit_l[p] == 1) out_l[p] = 2;
    if (out_r[p] == 1 && hit_r[p] == 1) out_r[p] = 2;
}

void launch_dcc(u8 *out_l, u8 *out_r, const float *disp_l, const float *disp_r, u8 *hit_l, u8 *hit_r, int H, int W)
{
    size_t HW = (size_t)H * W;
    STM_CHECK(hipMemsetAsync(hit_l, 1, HW, stream())); // d_dr_dcc.cu:107,111
    STM_CHECK(hipMemsetAsync(hit_r, 1, HW, stream()));
    STM_LAUNCH(stm_k_dcc_mark, dim3(cdiv(W, 256), H), dim3(256), 0, stream(), out_l, out_r, disp_l, disp_r, hit_l,
                       hit_r, H, W);
    STM_CHECK_LAUNCH();
    STM_LAUNCH(stm_k_dcc_merge, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, stream(), out_l, out_r, hit_l,
                       hit_r, HW);
    STM_CHECK_LAUNCH();
}

// The whole L/R check of one image row in one block (frame pipeline): both scatters stay inside the row, so the two
// hit maps live in LDS instead of in memset global planes, and every pixel's class (0, 1 mismatch, 2 occlusion)
// is written exactly once -- one launch instead of four memsets and two kernels, same classes (d_dr_dcc.cu:18-82).
__global__ __launch_bounds__(256) void stm_k_dcc_rows(u8 *__restrict__ out_l, u8 *__restrict__ out_r,
                                                      const float *__restrict__ disp_l, const float *__restrict__ disp_r, int W)
{
    extern __shared__ u8 dcc_lds[]; // hit_l[W] | hit_r[W] | flag_l[W] | flag_r[W]
    u8 *hit_l = dcc_lds, *hit_r = dcc_lds + W, *flag_l = dcc_lds + 2 * W, *flag_r = dcc_lds + 3 * W;
    const size_t row = (size_t)blockIdx.x * W;
    for (int x = threadIdx.x; x < W; x += 256) hit_l[x] = hit_r[x] = 1; // 1 = never hit (:107,111)
    __syncthreads();
    const float thresh = 1.0f; // :117
    for (int x = threadIdx.x; x < W; x += 256) {
        const float dl = disp_l[row + x];
        int c = min(max(x + (int)dl, 0), W - 1);
        flag_l[x] = fabsf(dl - disp_r[row + c]) > thresh;
        hit_r[c] = 0; // every writer stores 0
        const float dr = disp_r[row + x];
        c = min(max(x - (int)dr, 0), W - 1);
        flag_r[x] = fabsf(dr - disp_l[row + c]) > thresh;
        hit_l[c] = 0;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += 256) {
        out_l[row + x] = flag_l[x] ? (hit_l[x] ? 2 : 1) : 0;
        out_r[row + x] = flag_r[x] ? (hit_r[x] ? 2 : 1) : 0;
    }
}
// out_l / out_r need no initialisation: every pixel is written
void launch_dcc_rows(u8 *out_l, u8 *out_r, const float *disp_l, const float *disp_r, int H, int W)
{
    const size_t smem = 4 * (size_t)W;
    if (smem > 64 * 1024) STM_CHECK(hipFuncSetAttribute((const void *)stm_k_dcc_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    STM_LAUNCH(stm_k_dcc_rows, dim3(H), dim3(256), smem, stream(), out_l, out_r, disp_l, disp_r, W);
    STM_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ iterative region voting
// Outliers are few (2 % of a synthetic frame, ~15 % of a real one, fewer every iteration) but each one
// walks a cross region of ~600 pixels, so a thread per pixel leaves most lanes idle and a thread per
// outlier leaves most of the CHIP idle.  Here: (1) a compaction kernel lists the outlier pixels once;
// (2) per iteration a persistent grid of waves walks the list, one WAVE per outlier: one row of the cross
// region per step (lanes = pixels, coalesced), votes counted in a per-wave LDS histogram, the winner is a
// wave-wide max over (count, -bin), and the same wave applies the accept test.
// Every outlier's result is independent of the list order, so the atomic compaction is deterministic
// where it matters.  Histogram: max(D,65) bins (the reference's int[65] overflows for D > 65, A-Q17 ii).
// Both views of a frame go through every IRV launch together (blockIdx.y = view).
struct IrvArgs {
    float *disp[2];
    u8 *outl[2];
    const u8 *aU[2], *aD[2], *aL[2], *aR[2];
    uint32_t *list[2]; // outlier pixels in raster order; entries are retired in place (IV_ACCEPTED, IV_DEAD)
    int *counts[2];    // counts[v][0] = length of the list
    u8 *dirty[2];      // dirty[v][it][tile]: a pixel of the 64x64 tile was accepted in iteration it
    // per pixel, 16 bits: 1 + histogram bin of a reliable pixel, 0 = reliable with the bin out of range (counts towards the
    // region's size only), 0xFFFF = outlier (no vote).
    // Two planes: iteration `it` reads plane it & 1 (the state all its votes see, as the reference's separate vote
    // and apply kernels guarantee) and writes the pixels it accepts into the other plane.
    uint16_t *code[2][2];
    // vp[v][y][x], y in [0, H]: reliable (non-outlier) pixels, on the state BEFORE the first iteration, in the row segments of the
    // pixels (0 .. y - 1, x) -- a vertical prefix sum, so that the reliable pixels of a whole cross region are one subtraction
    const uint32_t *vp[2];
    // cnt[v][y][x]: reliable pixels of row y inside the row segment of pixel (y, x), same state (stm_k_dcc_irv_rows writes it,
    // stm_k_irv_compact_cm<true> sums it over a region's rows inside its tile: no vp plane on that path)
    const uint16_t *cnt[2];
    // device_diag(): bit 0 = an append past the list's capacity was dropped, bit 1 = the vote found a counter beyond the
    // capacity, bit 2 = a list entry that is neither retired nor a pixel of the frame.  None can happen while the counters are
    // cleared per call; the consumers clamp regardless (a replayed graph once ran with a stale counter, section 4 of DESIGN.md)
    // and this word makes a clamp VISIBLE: stm_last_error() reports and clears it.
    uint32_t *diag;
};
constexpr uint32_t IV_ACCEPTED = 0x80000000u; // list entry: pixel accepted in the previous iteration
constexpr uint32_t IV_DEAD = 0xFFFFFFFFu;     // list entry: nothing left to do
constexpr uint32_t IV_LATER = 0x40000000u;    // list entry: the first iteration cannot accept this pixel (its region holds <= thresh_s reliable pixels)

// vote code of one pixel: (int)disp + zero_disp is the histogram bin (d_dr_irv.cu:200-201)
constexpr uint32_t IV_NOVOTE = 0xFFFFu;
__device__ __forceinline__ uint16_t irv_code(u8 outl, float disp, int zd, int nb)
{
    if (outl != 0) return (uint16_t)IV_NOVOTE;
    // the conversion saturates (a caller's map may hold anything), so the sum saturates too: where (int)disp + zd leaves 32 bits
    // it stays at INT_MAX / INT_MIN, outside [0, nb) like the exact sum; everywhere else it is the exact sum
    const int b = __builtin_elementwise_add_sat((int)disp, zd);
    return (b >= 0 && b < nb) ? (uint16_t)(b + 1) : (uint16_t)0;
}
// f2i_sat(own) + zd as the float the accept ratio divides: the numerator where nothing in the region has a bin, and with nb - 1
// the bound of every numerator (see stm_k_irv_rowcount).  64 bits: own = INT_MAX (a map value of 2^31 or more) plus zd leaves 32.
__device__ __forceinline__ float irv_own_num(int own_i, int zd) { return (float)((long long)own_i + zd); }
// (float)max(nb - 1, f2i_sat(own) + zd): int -> float is monotone, so the maximum may be taken on the floats
__device__ __forceinline__ float irv_nmax(int nb, int own_i, int zd) { return fmaxf((float)(nb - 1), irv_own_num(own_i, zd)); }

// counters + dirty bytes of a frame, cleared by a kernel rather than hipMemsetAsync.  Round 2 saw stm_k_irv_vote fault
// (gpurun_out/r02i/gdb.txt: SIGSEGV in stm_k_irv_vote) only in test_frame_stream_graph_replay_survives_other_calls, i.e. only
// when the frame ran as a replayed hipGraph, in which this clear was the one memset node; with the clear as a kernel node the
// test passed.  That is circumstantial (the counter was never read back), so the consumers no longer trust the counter:
// stm_k_irv_compact drops appends past the list's capacity and stm_k_irv_vote clamps the length it walks.
__global__ __launch_bounds__(256) void stm_k_irv_clear(int *__restrict__ words, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) words[i] = 0;
}

// Pruning before the first iteration.  The reference accepts an outlier on (winning bin INDEX) / S > thresh_h (d_dr_irv.cu:36,
// SURVEY A-Q17 iv), S = the reliable pixels of its cross region.  The numerator never exceeds nmax = max(nb - 1, (int)own + zd),
// and S only grows from iteration to iteration (accepted pixels become reliable, nothing becomes unreliable): an outlier whose
// region ALREADY holds S0 reliable pixels with nmax / S0 <= thresh_h can never be accepted, whatever its votes, in any
// iteration (float division is monotone in both arguments, so the reference's test fails exactly when this one says so).  On a
// 1080p frame that is most outliers: regions of several hundred pixels against nmax / thresh_h = 160.  S0 of every pixel's
// region costs two image-sized passes:
//   stm_k_irv_rowcount:  cnt[y][x] = reliable pixels of row y inside the row segment of pixel (y, x)  (row prefix sums in LDS);
//   stm_k_irv_colprefix: vp[y][x]  = cnt[0][x] + .. + cnt[y - 1][x];  S0(y, x) = vp[y + armD + 1][x] - vp[y - armU][x].
// The compaction kernel then lists only the outliers that can still be accepted.
constexpr int IRC_W = 4; // waves per image row: each takes a quarter of the row (a one-wave block walked the row in eight dependent trips)
// `words` / `nwords`: the counters and dirty bytes of the call, cleared here (what stm_k_irv_clear does when there is no pruning pass;
// nothing reads them before stm_k_irv_compact)
__global__ __launch_bounds__(64 * IRC_W) void stm_k_irv_rowcount(IrvArgs a, uint16_t *__restrict__ cnt0, uint16_t *__restrict__ cnt1, int H, int W,
                                                                 int *__restrict__ words, int nwords)
{
    extern __shared__ uint32_t rp[]; // rp[x] = reliable pixels of this row in columns < x, x in [0, W]
    __shared__ int s_tot[IRC_W];
    const int v = blockIdx.y, y = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = (blockIdx.y * gridDim.x + blockIdx.x) * (64 * IRC_W) + threadIdx.x; i < nwords; i += gridDim.x * gridDim.y * (64 * IRC_W)) words[i] = 0;
    const u8 *__restrict__ outl = a.outl[v];
    const u8 *__restrict__ aL = a.aL[v], *__restrict__ aR = a.aR[v];
    uint16_t *__restrict__ cnt = (v ? cnt1 : cnt0) + (size_t)y * W;
    const size_t row = (size_t)y * W;
    const int Wq = (((W + IRC_W - 1) / IRC_W) + 63) & ~63; // columns per wave, a multiple of 64
    const int xb = wv * Wq, xe = min(W, xb + Wq);
    int carry = 0;
    if (threadIdx.x == 0) rp[0] = 0;
    for (int x0 = xb; x0 < xe; x0 += 256) { // four chunks of 64 per trip: their loads are in flight together
        u8 o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = outl[row + min(x0 + 64 * k + lane, W - 1)];
#pragma unroll
        for (int k = 0; k < 4; ++k) { // prefix inside a chunk = population count of the ballot below the lane (v_mbcnt)
            const int x = x0 + 64 * k + lane;
            const bool r = x < xe && o[k] == 0;
            const unsigned long long m = __ballot(r);
            const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (x < xe) rp[x + 1] = (uint32_t)(carry + below + (r ? 1 : 0)); // relative to the wave's first column
            carry += __popcll(m);
        }
    }
    if (lane == 0) s_tot[wv] = carry;
    __syncthreads();
    int off = 0; // reliable pixels left of this wave's part
    for (int q = 0; q < wv; ++q) off += s_tot[q];
    if (off)
        for (int x = xb + lane; x < xe; x += 64) rp[x + 1] += (uint32_t)off;
    __syncthreads();
    for (int x0 = xb; x0 < xe; x0 += 256) { // the row segment of the vote kernel: [x - armL, x + armR] clamped into the row
        int al[4], ar[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = min(x0 + 64 * k + lane, W - 1);
            al[k] = aL[row + x];
            ar[k] = aR[row + x];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + 64 * k + lane;
            if (x < xe) {
                const int cl = min(al[k], x);
                const int w = max(min(cl + ar[k] + 1, W - (x - cl)), 0);
                cnt[x] = (uint16_t)(rp[x - cl + w] - rp[x - cl]);
            }
        }
    }
}

// Frame pipeline: stm_k_dcc_rows and stm_k_irv_rowcount of both views in one block per image row.  Both are row-local and the
// second only re-read what the first had just written: here the two disparity rows are staged in LDS (the L/R check's gathers
// stay there), the classes never leave the block before they are final, the row prefix of `class == 0` is formed from them, and
// the outlier map, the 16-bit vote codes of both code planes (what stm_k_irv_compact_cm otherwise packs from the map and the
// disparities) and cnt leave once.  Eight waves: four per view, each with a quarter of the row as in stm_k_irv_rowcount.
// LDS: disparities float[2][W], rp u16[2][W + 1] (a row holds at most W < 65536 reliable pixels), hit bytes [2][W].
constexpr int DIR_T = 2 * 64 * IRC_W, DIR_PRE = 8;
static size_t dcc_irv_rows_lds(int W) { return 8 * (size_t)W + 4 * (size_t)(W + 1) + 2 * (size_t)W; }
__global__ __launch_bounds__(DIR_T) void stm_k_dcc_irv_rows(IrvArgs a, uint16_t *__restrict__ cnt0, uint16_t *__restrict__ cnt1, int H, int W,
                                                            int zd, int nb, int *__restrict__ words, int nwords)
{
    extern __shared__ float dir_lds[];
    __shared__ int s_tot[2][IRC_W];
    float *dsp_l = dir_lds, *dsp_r = dir_lds + W;
    uint16_t *rp0 = (uint16_t *)(dir_lds + 2 * W);
    u8 *hit_l = (u8 *)(rp0 + 2 * (W + 1)), *hit_r = hit_l + W;
    const int y = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = blockIdx.x * DIR_T + threadIdx.x; i < nwords; i += gridDim.x * DIR_T) words[i] = 0;
    const size_t row = (size_t)y * W;
    const int v = wave / IRC_W, wv = wave % IRC_W; // this wave's view and quarter of the row
    const int Wq = (((W + IRC_W - 1) / IRC_W) + 63) & ~63; // columns per wave, a multiple of 64
    const int xb = wv * Wq, xe = min(W, xb + Wq);
    // the horizontal arms of the wave's first DIR_PRE chunks (all of them up to W = 2048) are asked for now and used last
    const u8 *__restrict__ aL = a.aL[v], *__restrict__ aR = a.aR[v];
    int al[DIR_PRE], ar[DIR_PRE];
#pragma unroll
    for (int k = 0; k < DIR_PRE; ++k) {
        const int x = min(xb + 64 * k + lane, W - 1);
        al[k] = aL[row + x];
        ar[k] = aR[row + x];
    }
    for (int x = threadIdx.x; x < W; x += DIR_T) {
        dsp_l[x] = a.disp[0][row + x];
        dsp_r[x] = a.disp[1][row + x];
        hit_l[x] = hit_r[x] = 1; // 1 = never hit (d_dr_dcc.cu:107,111)
    }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += DIR_T) { // both scatters stay inside the row; every writer stores 0
        hit_r[min(max(x + (int)dsp_l[x], 0), W - 1)] = 0;
        hit_l[min(max(x - (int)dsp_r[x], 0), W - 1)] = 0;
    }
    __syncthreads();
    uint16_t *rp = rp0 + v * (W + 1);
    {
        const float *own = v ? dsp_r : dsp_l, *oth = v ? dsp_l : dsp_r;
        const u8 *hit = v ? hit_r : hit_l;
        u8 *__restrict__ outl = a.outl[v];
        uint16_t *__restrict__ code_a = a.code[v][0], *__restrict__ code_b = a.code[v][1];
        const float thresh = 1.0f; // d_dr_dcc.cu:117
        int carry = 0;
        if (lane == 0 && wv == 0) rp[0] = 0;
        for (int x0 = xb; x0 < xe; x0 += 64) { // prefix inside a chunk = population count of the ballot below the lane (v_mbcnt)
            const int x = x0 + lane, xc = min(x, W - 1);
            const float d = own[xc];
            const int c = min(max(v ? xc - (int)d : xc + (int)d, 0), W - 1);
            const u8 cls = fabsf(d - oth[c]) > thresh ? (hit[xc] ? 2 : 1) : 0; // 1 mismatch, 2 occlusion: never hit (d_dr_dcc.cu:18-82)
            const bool r = x < xe && cls == 0;
            const unsigned long long m = __ballot(r);
            const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (x < xe) {
                outl[row + x] = cls;
                code_a[row + x] = code_b[row + x] = irv_code(cls, d, zd, nb);
                rp[x + 1] = (uint16_t)(carry + below + (r ? 1 : 0)); // relative to the wave's first column
            }
            carry += __popcll(m);
        }
        if (lane == 0) s_tot[v][wv] = carry;
    }
    __syncthreads();
    int off = 0; // reliable pixels left of this wave's part
    for (int q = 0; q < wv; ++q) off += s_tot[v][q];
    if (off)
        for (int x = xb + lane; x < xe; x += 64) rp[x + 1] += (uint16_t)off;
    __syncthreads();
    uint16_t *__restrict__ cnt = (v ? cnt1 : cnt0) + row;
    // the row segment of the vote kernel: [x - armL, x + armR] clamped into the row
    auto count = [&](int x, int l, int r) {
        const int cl = min(l, x);
        const int w = max(min(cl + r + 1, W - (x - cl)), 0);
        cnt[x] = (uint16_t)(rp[x - cl + w] - rp[x - cl]);
    };
#pragma unroll
    for (int k = 0; k < DIR_PRE; ++k) {
        const int x = xb + 64 * k + lane;
        if (x < xe) count(x, al[k], ar[k]);
    }
    for (int x = xb + 64 * DIR_PRE + lane; x < xe; x += 64) count(x, aL[row + x], aR[row + x]);
}

constexpr int ICP_SEG = 16; // row segments per column block
__global__ __launch_bounds__(64 * ICP_SEG) void stm_k_irv_colprefix(const uint16_t *__restrict__ cnt0, const uint16_t *__restrict__ cnt1,
                                                                   uint32_t *__restrict__ vp0, uint32_t *__restrict__ vp1, int H, int W)
{
    __shared__ uint32_t part[ICP_SEG][64];
    const uint16_t *__restrict__ cnt = blockIdx.y ? cnt1 : cnt0;
    uint32_t *__restrict__ vp = blockIdx.y ? vp1 : vp0;
    const int lx = threadIdx.x & 63, seg = threadIdx.x >> 6, x = blockIdx.x * 64 + lx;
    const int rs = (H + ICP_SEG - 1) / ICP_SEG, y0 = seg * rs, y1 = min(H, y0 + rs);
    uint32_t sum = 0;
    if (x < W) {
        int y = y0;
        for (; y + 8 <= y1; y += 8) { // eight loads in flight
            uint32_t t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = cnt[(size_t)(y + k) * W + x];
#pragma unroll
            for (int k = 0; k < 8; ++k) sum += t[k];
        }
        for (; y < y1; ++y) sum += cnt[(size_t)y * W + x];
    }
    part[seg][lx] = sum;
    __syncthreads();
    if (x >= W) return;
    uint32_t run = 0;
    for (int s2 = 0; s2 < seg; ++s2) run += part[s2][lx];
    int y = y0;
    for (; y + 8 <= y1; y += 8) {
        uint32_t t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = cnt[(size_t)(y + k) * W + x];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            vp[(size_t)(y + k) * W + x] = run;
            run += t[k];
        }
    }
    for (; y < y1; ++y) {
        vp[(size_t)y * W + x] = run;
        run += cnt[(size_t)y * W + x];
    }
    if (y1 == H && y0 < H) vp[(size_t)H * W + x] = run; // the segment that ends the column also writes the total
}

// four pixels per thread (one dword of the u8 outlier map), 4096 pixels per block; the block's outliers are
// appended in raster order with ONE global atomic (the counter is a single address: per-wave atomics made this
// kernel atomic-bound)
constexpr int IC_T = 1024;
__global__ __launch_bounds__(IC_T) void stm_k_irv_compact(IrvArgs a, uint32_t HW, int zd, int nb, int H, int W, int usd, float thresh_h, int thresh_s)
{
    __shared__ int s_tot[IC_T / 64];
    __shared__ int s_base;
    const int v = blockIdx.y;
    const u8 *__restrict__ outl = a.outl[v];
    const float *__restrict__ disp = a.disp[v];
    uint32_t *__restrict__ list = a.list[v];
    const uint32_t p = (blockIdx.x * (uint32_t)IC_T + threadIdx.x) * 4u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t w = 0;
    // the same pass packs (outlier flag, disparity) into the 16-bit vote code the vote kernel reads:
    // one dword of flags + one float4 of disparities in, four codes (8 bytes) out per thread and plane
    if (p + 4 <= HW && ((((uintptr_t)outl) & 3) | (((uintptr_t)disp) & 15)) == 0) {
        w = *(const uint32_t *)(outl + p);
        const float4 d = *(const float4 *)(disp + p);
        const uint32_t c0 = irv_code((u8)(w & 0xff), d.x, zd, nb), c1 = irv_code((u8)((w >> 8) & 0xff), d.y, zd, nb);
        const uint32_t c2 = irv_code((u8)((w >> 16) & 0xff), d.z, zd, nb), c3 = irv_code((u8)(w >> 24), d.w, zd, nb);
        const uint2 cc = make_uint2(c0 | (c1 << 16), c2 | (c3 << 16));
        *(uint2 *)(a.code[v][0] + p) = cc; // the code planes are workspace memory: aligned
        *(uint2 *)(a.code[v][1] + p) = cc;
    } else if (p < HW) {
        for (uint32_t j = 0; j < 4 && p + j < HW; ++j) {
            const u8 o = outl[p + j];
            w |= (uint32_t)o << (8 * j);
            a.code[v][0][p + j] = a.code[v][1][p + j] = irv_code(o, disp[p + j], zd, nb);
        }
    }
    const uint32_t *__restrict__ vp = a.vp[v];
    uint32_t later = 0; // bit j: pixel p + j cannot be accepted in the first iteration (S0 <= thresh_s, d_dr_irv.cu:35): its vote is skipped there
    if (vp != nullptr && w != 0) { // outliers that can never be accepted are not listed (see stm_k_irv_rowcount)
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (((w >> (8 * j)) & 0xff) && p + j < HW) {
                const int q = (int)(p + j), gy = q / W, gx = q - gy * W;
                int cu = a.aU[v][q], cd = a.aD[v][q];
                if (cu > usd) cu = usd;   // the clamps of the vote kernel (d_dr_irv.cu:179-180)
                cu = min(cu, gy);
                cd = min(cd, H - 1 - gy);
                const int s0 = (int)(vp[(size_t)(gy + cd + 1) * W + gx] - vp[(size_t)(gy - cu) * W + gx]);
                const float nmax = irv_nmax(nb, (int)disp[q], zd);
                if (s0 > 0 && !(nmax / (float)s0 > thresh_h)) w &= ~(0xffu << (8 * j));
                else if (s0 <= thresh_s) later |= 1u << j;
            }
    }
    const int c = ((w & 0xff) != 0) + ((w & 0xff00) != 0) + ((w & 0xff0000) != 0) + ((w & 0xff000000u) != 0);
    int incl = c; // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_tot[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
#pragma unroll
        for (int i = 0; i < IC_T / 64; ++i) tot += s_tot[i];
        s_base = tot ? atomicAdd(&a.counts[v][0], tot) : 0;
    }
    __syncthreads();
    int k = s_base + incl - c;
    for (int i = 0; i < wave; ++i) k += s_tot[i];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if ((w >> (8 * j)) & 0xff) {
            if ((uint32_t)k < HW) list[k] = (p + j) | ((later >> j) & 1u ? IV_LATER : 0u); // the list holds HW entries: a counter that was not cleared can never write past it
            else atomicOr(a.diag, 1u); // (never on the timed path)
            ++k;
        }
}

constexpr int IV_WAVES = 2;     // waves per block
constexpr int IV_PX_PER_BLOCK = 256; // grid per view = pixels / this (see launch_irv)
constexpr int IV_U = 8;         // region rows whose loads are in flight together

// max / sum over the 64 lanes as a scalar, on the DPP path (six ALU ops with a DPP operand; lanes without a source keep
// their value / add 0): the LDS round trips of a shuffle reduction are what this kernel cannot afford
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
    asm volatile("s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1"
                 : "+v"(v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    // rotations inside the rows of 16 (DPP row_ror: every lane ends with its row's sum), then the four rows through readlane
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false);
    return (uint32_t)(__builtin_amdgcn_readlane((int)v, 0) + __builtin_amdgcn_readlane((int)v, 16) + __builtin_amdgcn_readlane((int)v, 32) +
                      __builtin_amdgcn_readlane((int)v, 48));
}

// Iteration `it` (0-based): vote (dr_irv_pre_kernel, d_dr_irv.cu:134-220) and apply (dr_irv_kernel_3, :17-43) for
// every live pixel of the outlier list.
// One wave per outlier, one region row per wave step (lanes = pixels of the row segment, coalesced), IV_U rows in flight
// together.  Round 3 (real image content has 6x the synthetic frame's outliers, and the round-2 kernel needed 15 scalar and
// 8 vector instructions per region row): a row now costs two v_readlane, six vector instructions, a load and an LDS atomic
// and no scalar arithmetic --
//  * the lanes of a chunk of 64 region rows hold each row's first-pixel BYTE OFFSET into the code plane and its width; a row
//    step broadcasts both with v_readlane, adds the lane's own 2 l, loads 16 bits (lanes past the segment read whatever
//    follows and are discarded by one v_cndmask);
//  * no ballot / population count / exec masking per row: EVERY lane does the LDS atomic; a lane without a vote (outside the
//    segment, or on an outlier) adds to a slot of its own behind the histogram, which nothing reads; the region's size S
//    (d_dr_irv.cu:203, reliable pixels only) is the sum of the histogram, taken once per outlier;
//  * four copies of the histogram (lane % 4): in smooth regions all lanes vote for one bin and the LDS atomic unit
//    serialises same-address adds (round-2 counters: 82 % of the LDS-active cycles were such conflicts).
// Apply in the same kernel: the reference votes for ALL outliers on one state and only then updates it.  Here the
// votes read code plane `it & 1`, which nothing writes during this launch; an accepted pixel is written to the
// disparity / outlier maps (no vote reads them) and to the OTHER code plane, and its list entry is tagged
// IV_ACCEPTED; the next launch, whose write plane still lacks that pixel, copies it over and retires the entry.
// The list is never re-compacted: it stays in raster order, so waves that run together work on neighbouring
// outliers whose cross regions overlap in cache (re-listing through atomics scrambled that and cost 40 %).
// Pruning: an outlier whose cross region saw no accepted pixel in the previous iteration would repeat its
// previous vote exactly (the vote is a pure function of the region) and be rejected again, so it is skipped;
// `dirty` holds one byte per tile (irv_plan: 16 x 16 up to usd 55 in a frame) and iteration.  The region's box is
// [x - harm, x + harm] x [y - up, y + down]: only the up arm is clamped to usd, so the horizontal half-width is the longest arm the
// arm planes can hold -- usd where the frame made them, a byte's 255 where a caller supplied the table (irv_plan picks the tile size
// so that the box is at most 8 tiles wide).  The down arm is not clamped either: a box of more than 64 tiles (more than a lane
// each) is not tested at all and the outlier votes.
// paper_ratio: accept on (winning COUNT) / S > thresh_h (Mei et al.) instead of the reference's (winning BIN INDEX) / S
// (d_dr_irv.cu:36, SURVEY A-Q17 iv); off by default.
__global__ __launch_bounds__(64 * IV_WAVES) void stm_k_irv_vote(IrvArgs a, int it, int thresh_s, float thresh_h, int H, int W,
                                                                int nb, int zd, int usd, int harm, int tiles_x, int tiles_y, int tile_sh, int paper_ratio)
{
    extern __shared__ uint32_t irv_lds[]; // per wave: uint4 slots[nb + 1 + 64]: slot 0 = "other", 1 + b = bin b, then one per lane
    const int v = blockIdx.y;
    float *__restrict__ disp = a.disp[v];
    const uint16_t *__restrict__ code_pl = a.code[v][it & 1];
    uint16_t *__restrict__ code_nx = a.code[v][(it & 1) ^ 1];
    const u8 *__restrict__ aL = a.aL[v], *__restrict__ aR = a.aR[v];
    uint32_t *__restrict__ list = a.list[v];
    const u8 *__restrict__ dirty = it > 0 ? a.dirty[v] + (size_t)(it - 1) * tiles_x * tiles_y : nullptr;
    u8 *__restrict__ dirty_out = a.dirty[v] + (size_t)it * tiles_x * tiles_y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nslot = nb + 1 + 64;
    uint32_t *hist = irv_lds + wave * nslot * 4;
    const uint32_t nv_slot = (uint32_t)(nb + 1 + lane);                 // this lane's own no-vote slot
    const uint32_t sub_addr = (uint32_t)((wave * nslot * 4 + (lane & 3)) * 4); // LDS byte address of copy lane % 4 of slot 0
    const uint32_t lane2 = 2u * lane;
    const int n_raw = a.counts[v][0];
    const int n = min(n_raw, H * W); // never past the list (capacity H W), whatever the counter holds
    if (n_raw > H * W && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.diag, 2u);
    const int stride = gridDim.x * IV_WAVES;
    int i = blockIdx.x * IV_WAVES + wave;
    uint32_t entry_next = i < n ? list[i] : IV_DEAD;
    for (; i < n; i += stride) {
        const uint32_t entry = (uint32_t)__builtin_amdgcn_readfirstlane((int)entry_next);
        entry_next = i + stride < n ? list[i + stride] : IV_DEAD; // in flight while this outlier is processed
        if ((entry & ~(IV_ACCEPTED | IV_LATER)) >= (uint32_t)(H * W)) { // IV_DEAD, or not a pixel of this frame (stale memory behind a wrong counter)
            if (entry != IV_DEAD && lane == 0) atomicOr(a.diag, 4u);
            continue;
        }
        if ((entry & IV_LATER) && it == 0) continue; // S <= thresh_s in this iteration: rejected whatever the votes (the flag is ignored afterwards)
        if (entry & IV_ACCEPTED) { // accepted by the previous launch: bring this launch's write plane up to date
            if (lane == 0) {
                const uint32_t q = entry & ~IV_ACCEPTED;
                code_nx[q] = code_pl[q];
                list[i] = IV_DEAD;
            }
            continue;
        }
        const int p = (int)(entry & ~IV_LATER);
        const int gy = p / W, gx = p - gy * W;
        int cu = a.aU[v][p], cd = a.aD[v][p];
        const float own = disp[p]; // needed only for the default vote at the very end: issued here so its latency is hidden
        if (cu > usd) cu = usd;   // d_dr_irv.cu:179-180
        cu = min(cu, gy);         // arms built by ca_cross never leave the image; these two clamps only keep a
        cd = min(cd, H - 1 - gy); // caller who passes inconsistent arms from reading outside the planes
        cu = __builtin_amdgcn_readfirstlane(cu);
        cd = __builtin_amdgcn_readfirstlane(cd);
        if (dirty) { // the region's box, [gx-harm, gx+harm] x [gy-cu, gy+cd] (see above the kernel): at most 8 tiles wide
            const int tx0 = max(gx - harm, 0) >> tile_sh, tx1 = min(gx + harm, W - 1) >> tile_sh;
            const int ty0 = (gy - cu) >> tile_sh, ty1 = (gy + cd) >> tile_sh;
            const int nx = tx1 - tx0 + 1, nt = nx * (ty1 - ty0 + 1);
            int d = nt > 64; // more tiles than lanes (a down arm beyond usd): do not prune
            if (nt <= 64 && lane < nt) d = dirty[(ty0 + lane / nx) * tiles_x + tx0 + lane % nx];
            if (__ballot(d != 0) == 0) continue; // same region contents as last time -> same vote -> rejected again
        }
        const int nrows = cu + cd + 1; // rows gy-cu .. gy+cd inclusive (SURVEY A-Q17 iii)
        const int y_top = gy - cu;
        for (int sl = lane; sl <= nb; sl += 64) *(uint4 *)(hist + sl * 4) = make_uint4(0, 0, 0, 0); // the per-lane slots are never read
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int jb = 0; jb < nrows; jb += 64) {
            // lane r of the chunk: row y_top + jb + r; segment [gx - armL, gx + armR] clamped into the image row (a no-op for
            // consistent arms): byte offset of its first pixel in the code plane, and its width (0 past the region)
            uint32_t roff = 0;
            int rw = 0;
            if (jb + lane < nrows) {
                const int q = (y_top + jb + lane) * W + gx;
                const int cl = min((int)aL[q], gx);
                rw = max(min(cl + (int)aR[q] + 1, W - (gx - cl)), 0);
                roff = 2u * (uint32_t)(q - cl);
            }
            const int jend = min(nrows - jb, 64); // wave-uniform
            if (__ballot(rw > 32) == 0) {
                // every row segment of this chunk fits half a wave (the common case on textured content): TWO region rows per step,
                // lanes 0-31 on row j, lanes 32-63 on row j + 1; each lane fetches its row's offset and width from the lane that
                // holds them (ds_bpermute: the LDS crossbar, no memory access, no scalar round trip)
                const int half4 = (lane >> 5) * 4;
                const uint32_t l2 = 2u * (uint32_t)(lane & 31);
                const int lw = lane & 31;
                for (int j0 = 0; j0 < jend; j0 += 2 * IV_U) { // j0 + 2 u + 1 <= 63: no wrap of the lane index (64 is a multiple of 2 IV_U)
                    uint32_t cdv[IV_U];
                    int wv[IV_U];
                    const int sel = half4 + 4 * j0;
#pragma unroll
                    for (int u = 0; u < IV_U; ++u) { // rows past jend: their lanes hold offset 0 / width 0
                        const uint32_t so = (uint32_t)__builtin_amdgcn_ds_bpermute(sel + 8 * u, (int)roff);
                        wv[u] = __builtin_amdgcn_ds_bpermute(sel + 8 * u, rw);
                        cdv[u] = *(const uint16_t *)((const char *)code_pl + (so + l2));
                    }
#pragma unroll
                    for (int u = 0; u < IV_U; ++u) {
                        const uint32_t c = lw < wv[u] ? cdv[u] : IV_NOVOTE;
                        const uint32_t slot = min(c, nv_slot);
                        atomicAdd(irv_lds + ((slot * 16u + sub_addr) >> 2), 1u);
                    }
                }
                continue; // next chunk of rows
            }
            for (int j0 = 0; j0 < jend; j0 += IV_U) {
                uint32_t cdv[IV_U];
#pragma unroll
                for (int u = 0; u < IV_U; ++u) { // the first 64 pixels of IV_U rows: all loads issued before any is consumed
                    const uint32_t so = (uint32_t)__builtin_amdgcn_readlane((int)roff, j0 + u); // rows past jend: lanes hold 0 / width 0
                    cdv[u] = *(const uint16_t *)((const char *)code_pl + (so + lane2));
                }
#pragma unroll
                for (int u = 0; u < IV_U; ++u) {
                    const int w = __builtin_amdgcn_readlane(rw, j0 + u);
                    const uint32_t c = lane < w ? cdv[u] : IV_NOVOTE;
                    const uint32_t slot = min(c, nv_slot); // a vote (c <= nb) or this lane's own slot
                    atomicAdd(irv_lds + ((slot * 16u + sub_addr) >> 2), 1u);
                }
            }
            if (__ballot(rw > 64) != 0) { // segments wider than 64 pixels (arm sum >= 64): rare
                for (int j = 0; j < jend; ++j) {
                    const int w = __builtin_amdgcn_readlane(rw, j);
                    const uint32_t so = (uint32_t)__builtin_amdgcn_readlane((int)roff, j);
                    for (int c0 = 64; c0 < w; c0 += 64) {
                        uint32_t c = IV_NOVOTE;
                        if (c0 + lane < w) c = *(const uint16_t *)((const char *)code_pl + (so + 2u * (uint32_t)c0 + lane2));
                        const uint32_t slot = min(c, nv_slot);
                        atomicAdd(irv_lds + ((slot * 16u + sub_addr) >> 2), 1u);
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // first bin with the strictly largest count (d_dr_irv.cu:206-215): max over (count, -bin); S = all reliable pixels
        uint32_t key = 0, tot = 0;
        for (int sl = lane; sl <= nb; sl += 64) {
            const uint4 h4 = *(const uint4 *)(hist + sl * 4);
            const uint32_t c = h4.x + h4.y + h4.z + h4.w;
            tot += c;
            const uint32_t k = (c << 16) | (uint32_t)(0xFFFF - (sl - 1));
            if (sl > 0 && c != 0 && k > key) key = k;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        key = wave_max_u32(key);
        const int total = (int)wave_sum_u32(tot);
        int max_d = (int)own; // default: own disparity (d_dr_irv.cu:182)
        if (key != 0) max_d = (0xFFFF - (int)(key & 0xFFFF)) - zd;
        // apply (d_dr_irv.cu:32-41): the ratio uses the winning BIN INDEX, not its count (:36, SURVEY A-Q17 iv)
        const float num = paper_ratio ? (float)(key >> 16) : irv_own_num(max_d, zd); // max_d + zd: the bin, or f2i_sat(own) + zd beyond 32 bits
        if (total > thresh_s && num / (float)total > thresh_h) {
            const uint16_t nc = irv_code(0, (float)max_d, zd, nb);
            if (lane == 0) {
                a.outl[v][p] = 0;
                disp[p] = (float)max_d;
                code_nx[p] = nc;
                dirty_out[(gy >> tile_sh) * tiles_x + (gx >> tile_sh)] = 1; // same value from every writer
                list[i] = (uint32_t)p | IV_ACCEPTED;
            }
        } else if (!paper_ratio && total > 0 && !(irv_nmax(nb, (int)own, zd) / (float)total > thresh_h)) {
            // S only grows and the numerator never exceeds this bound (see stm_k_irv_rowcount): rejected now = rejected for good
            if (lane == 0) list[i] = IV_DEAD;
        }
    }
}

// ------------------------------------------------------------------ round 4: column runs
// profiles/r04_pmc_irv.txt: on real image content the vote kernel is bound by its vector instructions (60 % of the SIMD-cycles of a
// launch), about 380 per listed outlier, half of them the walk over the ~36 rows of its cross region.  But the row segments of a
// region depend on the COLUMN only (row q contributes [x - armL(q, x), x + armR(q, x)], d_dr_irv.cu:186-199), so two outliers of
// one column share every row their vertical arms have in common -- and 88 % of the listed outliers have a listed outlier directly
// above them whose row range differs by 2.2 rows in the mean (tools/irv_stats.py: 5.7 M region rows per iteration, 0.5 M when
// each outlier starts from the histogram of the one above).  So:
//  * stm_k_irv_compact_cm lists the outliers tile by tile (64 x 64 pixels), COLUMN-major inside a tile;
//  * stm_k_irv_vote_cm gives a wave a few consecutive entries: it keeps the histogram of the last region it counted and, for
//    the next entry of the same column, removes the rows that left the range and adds the rows that entered it (one pass over at
//    most 64 such rows, each with its sign); anything else (another column, no overlap) is counted from scratch.
// Everything else -- flags in the list entries, the two code planes, dirty tiles, the accept rule -- is stm_k_irv_vote's.
constexpr int IVC_CH = 16; // most list entries per wave and trip (fewer when the list is short: the chip wants many more waves than it holds)

// TILE (frame pipeline, after stm_k_dcc_irv_rows): the vote codes are already written, and S0 comes from the tile's own column
// sums instead of from the full-height prefix plane vp: the block reads cnt for its 64 columns and the rows
// [64 ty - usd, 64 ty + 64 + usd) of the image, 16 row segments per column as stm_k_irv_colprefix does, and keeps the running
// sums in LDS (pf[i][c] = cnt of the rows before tile row i; 32 bits: a count is at most 2 usd + 1 and a column holds 64 + 2 usd
// of them).  S0 is the same subtraction.  launch_irv takes this form only while the (65 + 2 usd) x 64 dwords fit IC_PF_ROWS.
constexpr int IC_PF_ROWS = 224; // rows of pf, the total included: usd <= 79
template <bool TILE>
__global__ __launch_bounds__(IC_T) void stm_k_irv_compact_cm(IrvArgs a, uint32_t HW, int zd, int nb, int H, int W, int usd, float thresh_h, int thresh_s, int tiles_x)
{
    extern __shared__ uint32_t ic_pf[];
    __shared__ uint32_t s_part[TILE ? IC_T / 64 : 1][64];
    __shared__ int s_tot[IC_T / 64];
    __shared__ int s_base;
    __shared__ uint32_t s_flag[64][16]; // per pixel of the tile one byte: 0 = not listed, 1 = listed, 2 = listed, not in the first iteration
    const int v = blockIdx.y;
    const u8 *__restrict__ outl = a.outl[v];
    const float *__restrict__ disp = a.disp[v];
    uint32_t *__restrict__ list = a.list[v];
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = threadIdx.x >> 4, c4 = (threadIdx.x & 15) * 4;
    const int gy = ty * 64 + r, gx0 = tx * 64 + c4;
    const uint32_t p = (uint32_t)gy * (uint32_t)W + (uint32_t)gx0;
    const int nvalid = gy < H ? min(max(W - gx0, 0), 4) : 0; // pixels of this thread inside the image
    uint32_t w = 0;
    const int yb = max(ty * 64 - usd, 0), nr = min(ty * 64 + 64 + usd, H) - yb; // TILE: image rows [yb, yb + nr) feed pf
    if (TILE) {
        const uint16_t *__restrict__ cnt = a.cnt[v];
        const int gxc = tx * 64 + lane, rs = (nr + IC_T / 64 - 1) / (IC_T / 64); // wave = row segment, lane = column
        const int i0 = min(wave * rs, nr), i1 = min(i0 + rs, nr);
        constexpr int RS = (IC_PF_ROWS - 1 + IC_T / 64 - 1) / (IC_T / 64); // rs <= RS: a segment's counts stay in registers, all loads in flight together
        uint32_t t[RS];
#pragma unroll
        for (int k = 0; k < RS; ++k) t[k] = (gxc < W && i0 + k < i1) ? cnt[(size_t)(yb + i0 + k) * W + gxc] : 0u;
        if (nvalid == 4 && (W & 3) == 0 && (((uintptr_t)outl) & 3) == 0) w = *(const uint32_t *)(outl + p);
        else
            for (int j = 0; j < nvalid; ++j) w |= (uint32_t)outl[p + j] << (8 * j);
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < RS; ++k) sum += t[k];
        s_part[wave][lane] = sum;
        if (__syncthreads_or(w != 0)) { // a tile without outliers lists nothing and needs no sums
            uint32_t run = 0;
            for (int s2 = 0; s2 < wave; ++s2) run += s_part[s2][lane];
#pragma unroll
            for (int k = 0; k < RS; ++k)
                if (i0 + k < i1) {
                    ic_pf[(i0 + k) * 64 + lane] = run;
                    run += t[k];
                }
            if (i1 == nr) ic_pf[nr * 64 + lane] = run; // the total (every segment that ends the column holds the same value)
            __syncthreads();
        }
    } else if (nvalid == 4 && (W & 3) == 0 && ((((uintptr_t)outl) & 3) | (((uintptr_t)disp) & 15)) == 0) {
        // the same pass packs (outlier flag, disparity) into the 16-bit vote code the vote kernel reads
        w = *(const uint32_t *)(outl + p);
        const float4 d = *(const float4 *)(disp + p);
        const uint32_t c0 = irv_code((u8)(w & 0xff), d.x, zd, nb), c1 = irv_code((u8)((w >> 8) & 0xff), d.y, zd, nb);
        const uint32_t c2 = irv_code((u8)((w >> 16) & 0xff), d.z, zd, nb), c3 = irv_code((u8)(w >> 24), d.w, zd, nb);
        const uint2 cc = make_uint2(c0 | (c1 << 16), c2 | (c3 << 16));
        *(uint2 *)(a.code[v][0] + p) = cc; // the code planes are workspace memory: aligned
        *(uint2 *)(a.code[v][1] + p) = cc;
    } else {
        for (int j = 0; j < nvalid; ++j) {
            const u8 o = outl[p + j];
            w |= (uint32_t)o << (8 * j);
            a.code[v][0][p + j] = a.code[v][1][p + j] = irv_code(o, disp[p + j], zd, nb);
        }
    }
    const uint32_t *__restrict__ vp = a.vp[v];
    uint32_t later = 0; // bit j: pixel p + j cannot be accepted in the first iteration (S0 <= thresh_s, d_dr_irv.cu:35)
    if ((TILE || vp != nullptr) && w != 0) { // outliers that can never be accepted are not listed (see stm_k_irv_rowcount)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (((w >> (8 * j)) & 0xff) && j < nvalid) {
                const int q = (int)p + j, gx = gx0 + j;
                int cu = a.aU[v][q], cd = a.aD[v][q];
                if (cu > usd) cu = usd;   // the clamps of the vote kernel (d_dr_irv.cu:179-180)
                cu = min(cu, gy);
                cd = min(cd, H - 1 - gy);
                if (TILE) cd = min(cd, usd); // arms of the frame's own stm_k_cross_arms never exceed usd: this only keeps the read inside pf
                const int s0 = TILE ? (int)(ic_pf[(gy + cd + 1 - yb) * 64 + c4 + j] - ic_pf[(gy - cu - yb) * 64 + c4 + j])
                                    : (int)(vp[(size_t)(gy + cd + 1) * W + gx] - vp[(size_t)(gy - cu) * W + gx]);
                const float nmax = irv_nmax(nb, (int)disp[q], zd);
                if (s0 > 0 && !(nmax / (float)s0 > thresh_h)) w &= ~(0xffu << (8 * j));
                else if (s0 <= thresh_s) later |= 1u << j;
            }
    }
    uint32_t fl = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if ((w >> (8 * j)) & 0xff) fl |= (((later >> j) & 1u) ? 2u : 1u) << (8 * j);
    s_flag[r][c4 >> 2] = fl;
    __syncthreads();
    // column-major: thread t takes rows 4 (t % 16) .. + 3 of column t / 16
    const int col = threadIdx.x >> 4, r4 = (threadIdx.x & 15) * 4;
    uint32_t f[4];
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[j] = (s_flag[r4 + j][col >> 2] >> (8 * (col & 3))) & 0xffu;
        c += f[j] != 0;
    }
    int incl = c; // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_tot[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
#pragma unroll
        for (int i = 0; i < IC_T / 64; ++i) tot += s_tot[i];
        s_base = tot ? atomicAdd(&a.counts[v][0], tot) : 0;
    }
    __syncthreads();
    int k = s_base + incl - c;
    for (int i = 0; i < wave; ++i) k += s_tot[i];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (f[j]) {
            const uint32_t q = ((uint32_t)(ty * 64 + r4 + j) << 16) | (uint32_t)(tx * 64 + col); // (row, column): launch_irv checks H < 2^14, W < 2^16
            if ((uint32_t)k < HW) list[k] = q | (f[j] == 2 ? IV_LATER : 0u); // the list holds HW entries: a counter that was not cleared can never write past it
            else atomicOr(a.diag, 1u); // (never on the timed path)
            ++k;
        }
}

// amdgpu_waves_per_eu(7, 7): with the `harm` and `chunk` arguments the register allocation came out at 63 VGPRs instead of 65 and the
// vote on real content at 52.6 instead of 49.4 us per launch (kernel trace, 1080p); scheduled for seven waves per SIMD -- what 65
// VGPRs had meant -- region voting on that frame takes 0.299 ms against 0.292 before the arguments (0.315 without the attribute)
__global__ __launch_bounds__(64 * IV_WAVES) __attribute__((amdgpu_waves_per_eu(7, 7))) void stm_k_irv_vote_cm(IrvArgs a, int it, int thresh_s, float thresh_h, int H, int W,
                                                                   int nb, int zd, int usd, int harm, int tiles_x, int tiles_y, int tile_sh, int paper_ratio, int chunk)
{
    extern __shared__ uint32_t irv_lds[]; // per wave: uint4 slots[nb + 1 + 64]: slot 0 = "other", 1 + b = bin b, then one per lane
    const int v = blockIdx.y;
    float *__restrict__ disp = a.disp[v];
    const uint16_t *__restrict__ code_pl = a.code[v][it & 1];
    uint16_t *__restrict__ code_nx = a.code[v][(it & 1) ^ 1];
    const u8 *__restrict__ aL = a.aL[v], *__restrict__ aR = a.aR[v];
    uint32_t *__restrict__ list = a.list[v];
    const u8 *__restrict__ dirty = it > 0 ? a.dirty[v] + (size_t)(it - 1) * tiles_x * tiles_y : nullptr;
    u8 *__restrict__ dirty_out = a.dirty[v] + (size_t)it * tiles_x * tiles_y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nslot = nb + 1 + 64;
    uint32_t *hist = irv_lds + wave * nslot * 4;
    const uint32_t nv_slot = (uint32_t)(nb + 1 + lane);                 // this lane's own no-vote slot
    const uint32_t sub_addr = (uint32_t)((wave * nslot * 4 + (lane & 3)) * 4); // LDS byte address of copy lane % 4 of slot 0
    const int n_raw = a.counts[v][0];
    const int n = min(n_raw, H * W); // never past the list (capacity H W), whatever the counter holds
    if (n_raw > H * W && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.diag, 2u);
    // entries per trip (1080p, real content: 5; 4 to 16 measured alike, 16 slower); chunk: stm_set_irv_chunk's 1 .. IVC_CH, 0 = this rule
    const int chl = chunk > 0 ? min(chunk, IVC_CH) : max(1, min(IVC_CH, n >> 14));
    const int nchunks = (n + chl - 1) / chl, stride = gridDim.x * IV_WAVES;
    const int half4 = (lane >> 5) * 4, lw = lane & 31;
    const uint32_t l2h = 2u * (uint32_t)lw, lane2 = 2u * lane;

    // `cnt` rows (cnt <= 64, wave-uniform): lane r < cnt holds row yrow of column gx and the sign sg (+1 / -1) its pixels are
    // counted with.  The row steps are stm_k_irv_vote's (two rows per step when every segment fits half a wave)
    auto count_rows = [&](int gx, int yrow, int sg, int cnt) {
        uint32_t roff = 0;
        int rw = 0;
        if (lane < cnt) {
            const int q = yrow * W + gx;
            const int cl = min((int)aL[q], gx);
            rw = max(min(cl + (int)aR[q] + 1, W - (gx - cl)), 0);
            roff = 2u * (uint32_t)(q - cl);
        }
        if (__ballot(rw > 32) == 0) {
            auto steps = [&](auto U_) {
                constexpr int U = decltype(U_)::value;
                for (int j0 = 0; j0 < cnt; j0 += 2 * U) {
                    uint32_t cdv[U];
                    int wv[U], sv[U];
                    const int sel = half4 + 4 * j0;
#pragma unroll
                    for (int u = 0; u < U; ++u) { // rows past cnt: their lanes hold offset 0 / width 0
                        const uint32_t so = (uint32_t)__builtin_amdgcn_ds_bpermute(sel + 8 * u, (int)roff);
                        wv[u] = __builtin_amdgcn_ds_bpermute(sel + 8 * u, rw);
                        sv[u] = __builtin_amdgcn_ds_bpermute(sel + 8 * u, sg);
                        cdv[u] = *(const uint16_t *)((const char *)code_pl + (so + l2h));
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const uint32_t c = lw < wv[u] ? cdv[u] : IV_NOVOTE;
                        const uint32_t slot = min(c, nv_slot);
                        atomicAdd(irv_lds + ((slot * 16u + sub_addr) >> 2), (uint32_t)sv[u]);
                    }
                }
            };
            // one trip (one load latency) for the few rows of an update; (64 is a multiple of 2 U: no wrap of the lane index)
            if (cnt <= 4) steps(std::integral_constant<int, 2>());
            else if (cnt <= 8) steps(std::integral_constant<int, 4>());
            else steps(std::integral_constant<int, IV_U>());
            return;
        }
        for (int j0 = 0; j0 < cnt; j0 += IV_U) {
            uint32_t cdv[IV_U];
#pragma unroll
            for (int u = 0; u < IV_U; ++u) { // the first 64 pixels of IV_U rows: all loads issued before any is consumed
                const uint32_t so = (uint32_t)__builtin_amdgcn_readlane((int)roff, (j0 + u) & 63); // rows past cnt: lanes hold 0 / width 0
                cdv[u] = *(const uint16_t *)((const char *)code_pl + (so + lane2));
            }
#pragma unroll
            for (int u = 0; u < IV_U; ++u) {
                const int w = __builtin_amdgcn_readlane(rw, (j0 + u) & 63);
                const int s1 = __builtin_amdgcn_readlane(sg, (j0 + u) & 63);
                const uint32_t c = lane < w ? cdv[u] : IV_NOVOTE;
                const uint32_t slot = min(c, nv_slot); // a vote (c <= nb) or this lane's own slot
                atomicAdd(irv_lds + ((slot * 16u + sub_addr) >> 2), (uint32_t)s1);
            }
        }
        if (__ballot(rw > 64) != 0) { // segments wider than 64 pixels (arm sum >= 64): rare
            for (int j = 0; j < cnt; ++j) {
                const int w = __builtin_amdgcn_readlane(rw, j);
                const uint32_t so = (uint32_t)__builtin_amdgcn_readlane((int)roff, j);
                const int s1 = __builtin_amdgcn_readlane(sg, j);
                for (int c0 = 64; c0 < w; c0 += 64) {
                    uint32_t c = IV_NOVOTE;
                    if (c0 + lane < w) c = *(const uint16_t *)((const char *)code_pl + (so + 2u * (uint32_t)c0 + lane2));
                    const uint32_t slot = min(c, nv_slot);
                    atomicAdd(irv_lds + ((slot * 16u + sub_addr) >> 2), (uint32_t)s1);
                }
            }
        }
    };

    for (int ch = blockIdx.x * IV_WAVES + wave; ch < nchunks; ch += stride) {
        // the chunk's entries and their pixels' vertical arms and disparities: one gather each for the whole chunk
        const int i0 = ch * chl;
        uint32_t e_l = IV_DEAD;
        int cu_l = 0, cd_l = 0;
        float own_l = 0.f;
        if (lane < chl && i0 + lane < n) {
            e_l = list[i0 + lane];
            const uint32_t yx = e_l & ~(IV_ACCEPTED | IV_LATER), q = (yx >> 16) * (uint32_t)W + (yx & 0xffffu);
            if ((yx >> 16) < (uint32_t)H && (yx & 0xffffu) < (uint32_t)W) {
                cu_l = a.aU[v][q];
                cd_l = a.aD[v][q];
                own_l = disp[q];
            }
        }
        bool have = false; // the LDS histogram holds rows r0 .. r1 of column rx
        int rx = 0, r0 = 0, r1 = 0;
        for (int k = 0; k < chl && i0 + k < n; ++k) {
            const int i = i0 + k;
            const uint32_t entry = (uint32_t)__builtin_amdgcn_readlane((int)e_l, k);
            const int gy = (int)((entry & ~(IV_ACCEPTED | IV_LATER)) >> 16), gx = (int)(entry & 0xffffu); // entries are (row << 16 | column)
            if (gy >= H || gx >= W) { // IV_DEAD, or not a pixel of this frame (stale memory behind a wrong counter)
                if (entry != IV_DEAD && lane == 0) atomicOr(a.diag, 4u);
                continue;
            }
            const int p = gy * W + gx;
            if ((entry & IV_LATER) && it == 0) continue; // S <= thresh_s in this iteration: rejected whatever the votes (the flag is ignored afterwards)
            if (entry & IV_ACCEPTED) { // accepted by the previous launch: bring this launch's write plane up to date
                if (lane == 0) {
                    code_nx[p] = code_pl[p];
                    list[i] = IV_DEAD;
                }
                continue;
            }
            int cu = __builtin_amdgcn_readlane(cu_l, k), cd = __builtin_amdgcn_readlane(cd_l, k);
            const float own = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, own_l), k));
            if (cu > usd) cu = usd;   // d_dr_irv.cu:179-180
            cu = min(cu, gy);         // arms built by ca_cross never leave the image; these two clamps only keep a
            cd = min(cd, H - 1 - gy); // caller who passes inconsistent arms from reading outside the planes
            if (dirty) { // the region's box, [gx-harm, gx+harm] x [gy-cu, gy+cd] (see stm_k_irv_vote): at most 8 tiles wide
                const int tx0 = max(gx - harm, 0) >> tile_sh, tx1 = min(gx + harm, W - 1) >> tile_sh;
                const int ty0 = (gy - cu) >> tile_sh, ty1 = (gy + cd) >> tile_sh;
                const int nx = tx1 - tx0 + 1, nt = nx * (ty1 - ty0 + 1);
                int d = nt > 64; // more tiles than lanes (a down arm beyond usd): do not prune
                const int lq = (lane * ((0x10000 + nx - 1) / nx)) >> 16; // lane / nx for lane < 64, nx <= 8 (the scalar unit divides once)
                if (nt <= 64 && lane < nt) d = dirty[(ty0 + lq) * tiles_x + tx0 + (lane - lq * nx)];
                if (__ballot(d != 0) == 0) continue; // same region contents as last time -> same vote -> rejected again
            }
            const int t0 = gy - cu, t1 = gy + cd; // rows t0 .. t1 inclusive (SURVEY A-Q17 iii)
            const int nrows = t1 - t0 + 1;
            // rows that leave / enter the range when the histogram of rows r0 .. r1 of this column is kept
            const int rem_top = max(min(t0, r1 + 1) - r0, 0), add_top = max(min(r0, t1 + 1) - t0, 0);
            const int rem_bot = max(r1 - max(t1, r0 - 1), 0), add_bot = max(t1 - max(r1, t0 - 1), 0);
            const int nd = rem_top + add_top + rem_bot + add_bot;
            if (have && gx == rx && max(t0, r0) <= min(t1, r1) && nd < nrows && nd <= 64) {
                if (nd > 0) {
                    int yrow = 0, sg = 0, j = lane;
                    if (j < rem_top) { yrow = r0 + j; sg = -1; }
                    else if ((j -= rem_top) < add_top) { yrow = t0 + j; sg = 1; }
                    else if ((j -= add_top) < rem_bot) { yrow = t1 + 1 + j; sg = -1; }
                    else if ((j -= rem_bot) < add_bot) { yrow = r1 + 1 + j; sg = 1; }
                    count_rows(gx, yrow, sg, nd);
                }
            } else {
                for (int sl = lane; sl <= nb; sl += 64) *(uint4 *)(hist + sl * 4) = make_uint4(0, 0, 0, 0); // the per-lane slots are never read
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int jb = 0; jb < nrows; jb += 64) count_rows(gx, t0 + jb + lane, 1, min(nrows - jb, 64));
            }
            have = true; rx = gx; r0 = t0; r1 = t1;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // first bin with the strictly largest count (d_dr_irv.cu:206-215): max over (count, -bin); S = all reliable pixels
            uint32_t key = 0, tot = 0;
            for (int sl = lane; sl <= nb; sl += 64) {
                const uint4 h4 = *(const uint4 *)(hist + sl * 4);
                const uint32_t c = h4.x + h4.y + h4.z + h4.w;
                tot += c;
                const uint32_t kk = (c << 16) | (uint32_t)(0xFFFF - (sl - 1));
                if (sl > 0 && c != 0 && kk > key) key = kk;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            key = wave_max_u32(key);
            const int total = (int)wave_sum_u32(tot);
            int max_d = (int)own; // default: own disparity (d_dr_irv.cu:182)
            if (key != 0) max_d = (0xFFFF - (int)(key & 0xFFFF)) - zd;
            // apply (d_dr_irv.cu:32-41): the ratio uses the winning BIN INDEX, not its count (:36, SURVEY A-Q17 iv)
            const float num = paper_ratio ? (float)(key >> 16) : irv_own_num(max_d, zd); // max_d + zd: the bin, or f2i_sat(own) + zd beyond 32 bits
            if (total > thresh_s && num / (float)total > thresh_h) {
                const uint16_t nc = irv_code(0, (float)max_d, zd, nb);
                if (lane == 0) {
                    a.outl[v][p] = 0;
                    disp[p] = (float)max_d;
                    code_nx[p] = nc;
                    dirty_out[(gy >> tile_sh) * tiles_x + (gx >> tile_sh)] = 1; // same value from every writer
                    list[i] = (entry & ~IV_LATER) | IV_ACCEPTED;
                }
            } else if (!paper_ratio && total > 0 && !(irv_nmax(nb, (int)own, zd) / (float)total > thresh_h)) {
                // S only grows and the numerator never exceeds this bound (see stm_k_irv_rowcount): rejected now = rejected for good
                if (lane == 0) list[i] = IV_DEAD;
            }
        }
    }
}

// The dispatch of launch_irv, as host arithmetic: stm_irv_path (stm_hip.h) reports it, launch_irv runs it.
struct IrvPlan {
    int rounds;  // vote launches
    int harm;    // the longest horizontal arm the arm planes can hold: the half-width of the dirty box
    int tile_sh; // log2 of the dirty tiles' edge
    int chunk;   // stm_set_irv_chunk's value where the column-run kernel votes, else 0
    bool prune, runs, chain;
};
static IrvPlan irv_plan(int H, int W, int usd, int iterations, bool device_flavour, bool with_dcc)
{
    IrvPlan pl;
    const size_t HW = (size_t)H * W;
    // host flavour (d_dr_irv.cu:344-353): one vote, then `iterations` applies of which only the first can change anything
    pl.rounds = device_flavour ? std::max(iterations, 0) : (iterations > 0 ? 1 : 0);
    // dirty tiles: the smallest power of two >= 16 for which a region's bounding box spans at most 8 x 8 tiles.  Vertically the box
    // is the region's own rows (the up arm is clamped to usd, d_dr_irv.cu:179-180).  Horizontally nothing clamps the arms (neither
    // here nor in the reference): the frame's own stm_k_cross_arms never makes one longer than usd, a caller's table (dr_irv,
    // d_dr_irv) holds bytes, so the box is [x - harm, x + harm] cut to the image row
    const int us = std::min(std::max(usd, 0), 255);
    pl.harm = with_dcc ? us : 255;
    pl.tile_sh = 4;
    while ((2 * us) / (1 << pl.tile_sh) + 2 > 8) ++pl.tile_sh; // (the frame: this alone, as it always was)
    while (std::min(2 * pl.harm, W - 1) / (1 << pl.tile_sh) + 2 > 8) ++pl.tile_sh;
    // pruning tables (stm_k_irv_rowcount): not with the paper's accept rule (its numerator is a count: no such bound)
    pl.prune = !irv_paper_ratio() && W <= 16000;
    // round 4: the list column-major inside 64 x 64 tiles, a wave votes for runs of a column incrementally; 300: the raster list of round 3
    // (also for frames too large for the (row, column) entries of the new list)
    pl.runs = (agg_variant() / 100) % 10 != 3 && H < (1 << 14) && W < (1 << 16);
    // the frame's short chain: L/R check + row counts + vote codes in one row kernel, column sums inside the compaction kernel
    // (no stm_k_irv_colprefix, no vp plane); 600: the separate kernels
    pl.chain = with_dcc && pl.prune && pl.runs && pl.rounds > 0 && HW < IV_LATER && (agg_variant() / 100) % 10 != 6 &&
               65 + 2 * std::min(usd, 255) <= IC_PF_ROWS && dcc_irv_rows_lds(W) <= 64 * 1024;
    pl.chunk = pl.runs ? irv_chunk() : 0;
    return pl;
}
int irv_path(int H, int W, int usd, int iterations, bool device_flavour, bool with_dcc)
{
    const IrvPlan pl = irv_plan(H, W, usd, iterations, device_flavour, with_dcc);
    return (pl.prune ? 1 : 0) | (pl.runs ? 2 : 0) | (pl.chain ? 4 : 0) | (pl.tile_sh << 8) | (pl.chunk << 16);
}

void launch_irv(int nviews, float *const *disp, u8 *const *outl, const u8 *const *up, const u8 *const *down,
                const u8 *const *left, const u8 *const *right, int thresh_s, float thresh_h, int H, int W, int D, int zd,
                int usd, int iterations, bool device_flavour, bool with_dcc)
{
    const size_t HW = (size_t)H * W;
    const int nb = D > 65 ? D : 65;
    if (nviews < 1 || nviews > 2 || (with_dcc && nviews != 2)) {
        fail("launch_irv: 1 or 2 views (2 with the L/R check)", "nviews", __FILE__, __LINE__);
        return; // only reached in error mode 1
    }
    const IrvPlan pl = irv_plan(H, W, usd, iterations, device_flavour, with_dcc);
    const int rounds = pl.rounds, tile_sh = pl.tile_sh;
    const bool prune = pl.prune, runs = pl.runs, chain = pl.chain;
    IrvArgs a;
    const int tiles_x = cdiv(W, 1 << tile_sh), tiles_y = cdiv(H, 1 << tile_sh);
    const size_t dirty_sz = (size_t)(rounds + 1) * tiles_x * tiles_y;
    const size_t ncount = 4; // per view: list length
    const size_t nwords = ncount + (2 * dirty_sz + 3) / 4;
    int *counts = Workspace::get<int>(nwords); // counters, then dirty bytes: cleared together
    for (int v = 0; v < 2; ++v) {
        const int s = v < nviews ? v : 0;
        a.disp[v] = disp[s]; a.outl[v] = outl[s];
        a.aU[v] = up[s]; a.aD[v] = down[s]; a.aL[v] = left[s]; a.aR[v] = right[s];
        a.counts[v] = counts + 2 * v;
        a.dirty[v] = (u8 *)(counts + ncount) + (size_t)v * dirty_sz;
    }
    for (int v = 0; v < nviews; ++v) {
        a.list[v] = Workspace::get<uint32_t>(HW);
        a.code[v][0] = Workspace::get<uint16_t>(HW + 64); // + 64: a row's 64-lane load may run past the last segment (its lanes are discarded)
        a.code[v][1] = Workspace::get<uint16_t>(HW + 64);
    }
    if (nviews == 1) { a.list[1] = a.list[0]; a.code[1][0] = a.code[0][0]; a.code[1][1] = a.code[0][1]; }
    uint16_t *cnt[2] = {nullptr, nullptr};
    uint32_t *vp[2] = {nullptr, nullptr};
    if (prune)
        for (int v = 0; v < nviews; ++v) {
            cnt[v] = Workspace::get<uint16_t>(HW);
            if (!chain) vp[v] = Workspace::get<uint32_t>(HW + W);
        }
    a.vp[0] = vp[0];
    a.vp[1] = nviews == 2 ? vp[1] : vp[0];
    a.cnt[0] = cnt[0];
    a.cnt[1] = nviews == 2 ? cnt[1] : cnt[0];
    a.diag = device_diag();
    if (with_dcc && !chain) launch_dcc_rows(outl[0], outl[1], disp[0], disp[1], H, W);
    if (rounds == 0) return; // nothing observable happens (a host-flavour vote without an apply only fills scratch)
    if (HW >= IV_LATER) {
        fail("dr_irv: more than 2^30 - 1 pixels", "num_rows * num_cols", __FILE__, __LINE__);
        return;
    }
    ProfScope p("irv");
    if (!prune) {
        STM_LAUNCH(stm_k_irv_clear, dim3((unsigned)cdiv((int)nwords, 256)), dim3(256), 0, stream(), counts, (int)nwords);
        STM_CHECK_LAUNCH();
    }
    if (chain) {
        STM_LAUNCH(stm_k_dcc_irv_rows, dim3(H), dim3(DIR_T), dcc_irv_rows_lds(W), stream(), a, cnt[0], cnt[1], H, W, zd, nb, counts, (int)nwords);
        STM_CHECK_LAUNCH();
    } else if (prune) {
        STM_LAUNCH(stm_k_irv_rowcount, dim3(H, nviews), dim3(64 * IRC_W), (size_t)(W + 1) * 4, stream(), a, cnt[0], nviews == 2 ? cnt[1] : cnt[0], H, W,
                   counts, (int)nwords);
        STM_CHECK_LAUNCH();
        STM_LAUNCH(stm_k_irv_colprefix, dim3(cdiv(W, 64), nviews), dim3(64 * ICP_SEG), 0, stream(), cnt[0], nviews == 2 ? cnt[1] : cnt[0], vp[0],
                   nviews == 2 ? vp[1] : vp[0], H, W);
        STM_CHECK_LAUNCH();
    }
    if (chain) {
        const int t64x = cdiv(W, 64), t64y = cdiv(H, 64), us = std::min(usd, 255); // (arms are bytes)
        STM_LAUNCH(stm_k_irv_compact_cm<true>, dim3((unsigned)(t64x * t64y), nviews), dim3(IC_T), (size_t)(65 + 2 * us) * 64 * 4, stream(), a, (uint32_t)HW,
                   zd, nb, H, W, us, thresh_h, thresh_s, t64x);
    } else if (runs) {
        const int t64x = cdiv(W, 64), t64y = cdiv(H, 64);
        STM_LAUNCH(stm_k_irv_compact_cm<false>, dim3((unsigned)(t64x * t64y), nviews), dim3(IC_T), 0, stream(), a, (uint32_t)HW, zd, nb, H, W, usd, thresh_h,
                   thresh_s, t64x);
    } else {
        STM_LAUNCH(stm_k_irv_compact, dim3((unsigned)((HW + 4 * IC_T - 1) / (4 * IC_T)), nviews), dim3(IC_T), 0, stream(), a, (uint32_t)HW, zd,
                           nb, H, W, usd, thresh_h, thresh_s);
    }
    STM_CHECK_LAUNCH();
    const size_t smem = (size_t)(nb + 1 + 64) * 16 * IV_WAVES; // per wave: four copies of (other, nb bins), one slot per lane
    // Several times more waves than the chip holds (1080p: 8100 blocks of 2 waves per view for 8192 wave slots): the waves walk
    // the list with a fixed stride and outliers differ a lot in work, so freed slots must be refilled by the dispatcher --
    // with exactly one resident grid (1024 blocks of 4 waves) the vote took 0.36 ms per frame, with 4096 such blocks 0.30,
    // with 8100 blocks of 2 waves 0.29 (16384 blocks of 4: 0.32; single-wave blocks: no further gain)
    const int iv_blocks = (int)std::min<size_t>(std::max<size_t>((HW + IV_PX_PER_BLOCK - 1) / IV_PX_PER_BLOCK, 256), 32768);
    for (int it = 0; it < rounds; ++it) {
        if (runs)
            STM_LAUNCH(stm_k_irv_vote_cm, dim3(iv_blocks, nviews), dim3(64 * IV_WAVES), smem, stream(), a, it, thresh_s, thresh_h, H,
                               W, nb, zd, usd, pl.harm, tiles_x, tiles_y, tile_sh, irv_paper_ratio(), pl.chunk);
        else
            STM_LAUNCH(stm_k_irv_vote, dim3(iv_blocks, nviews), dim3(64 * IV_WAVES), smem, stream(), a, it, thresh_s, thresh_h, H,
                               W, nb, zd, usd, pl.harm, tiles_x, tiles_y, tile_sh, irv_paper_ratio());
        STM_CHECK_LAUNCH();
    }
}

// ------------------------------------------------------------------ stencils, fast path
// Compile-time radius, four adjacent output pixels per thread: a tile row is read once as aligned float4s and
// reused by the four pixels (LDS reads per tap drop 4x), the spatial weights are wave-uniform and come in through
// scalar loads (no LDS slot, no VGPR), taps are accumulated per pixel in the reference's row-major order.
constexpr int SF_TX = 16, SF_TY = 16; // threads; a block covers 64 x 16 output pixels

template <int R>
__global__ __launch_bounds__(SF_TX *SF_TY) void stm_k_gaussian_max_r(const float *__restrict__ in, float *__restrict__ out,
                                                                    const float *__restrict__ spatial, float norm, int H, int W,
                                                                    int invert)
{
    constexpr int KW = 2 * R + 1, NF = (KW + 3 + 3) / 4 * 4; // floats a thread needs per tile row, rounded to float4s
    constexpr int TW = (SF_TX * 4 + 2 * R + 3) / 4 * 4 + 4, TH = SF_TY + 2 * R;
    __shared__ float4 tile4[TH * TW / 4];
    float *tile = (float *)tile4;
    const int tid = threadIdx.y * SF_TX + threadIdx.x;
    const int x0 = blockIdx.x * SF_TX * 4, y0 = blockIdx.y * SF_TY;
    // A tile (with its halo) that holds one value c in {0, 1} -- most tiles of an occlusion mask: 84 % / 75 % on the synthetic / real
    // 1080p frame -- needs no stencil: every pixel's sum is 0, or (c = 1) the weights added in tap order, which is exactly how
    // `norm` was formed (stencil_norm), so the quotient is exactly c and max(c, c) = c
    float c0;
    {
        const float v0 = in[(size_t)min(max(y0 - R, 0), H - 1) * W + min(max(x0 - R, 0), W - 1)];
        c0 = invert ? 1.0f - v0 : v0;
    }
    int differs = 0;
    for (int i = tid; i < TH * TW; i += SF_TX * SF_TY) {
        const int ty = i / TW, tx = i - ty * TW;
        const int gx = min(max(x0 + tx - R, 0), W - 1), gy = min(max(y0 + ty - R, 0), H - 1); // clamp border (d_filter_gaussian.cu:39)
        const float v = in[(size_t)gy * W + gx];
        const float tv = invert ? 1.0f - v : v;
        tile[i] = tv;
        differs |= tv != c0;
    }
    const bool one_value = __syncthreads_or(differs) == 0 && (c0 == 0.0f || c0 == 1.0f); // block-uniform
    const int gx = x0 + threadIdx.x * 4, gy = y0 + threadIdx.y;
    if (gx >= W || gy >= H) return;
    if (one_value) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (gx + i < W) out[(size_t)gy * W + gx + i] = c0;
        return;
    }
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 acc[2] = {{0.f, 0.f}, {0.f, 0.f}}; // pixel pairs (0,1) and (2,3): v_pk_mul_f32 / v_pk_add_f32, same rounding per component
    for (int y = 0; y < KW; ++y) {
        float row[NF];
        const float4 *src = (const float4 *)(tile + (threadIdx.y + y) * TW + threadIdx.x * 4);
#pragma unroll
        for (int j = 0; j < NF / 4; ++j) {
            const float4 t = src[j];
            row[4 * j] = t.x; row[4 * j + 1] = t.y; row[4 * j + 2] = t.z; row[4 * j + 3] = t.w;
        }
        const float *krow = spatial + y * KW; // uniform address -> scalar loads
#pragma unroll
        for (int x = 0; x < KW; ++x) {
            const float w = krow[x];
            const f2 w2 = {w, w};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f2 v = {row[x + 2 * h], row[x + 2 * h + 1]};
                const f2 t = v * w2;
                acc[h] = acc[h] + t;
            }
        }
    }
    const float res[4] = {acc[0].x, acc[0].y, acc[1].x, acc[1].y};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (gx + i < W) {
            const float va = tile[(threadIdx.y + R) * TW + threadIdx.x * 4 + i + R];
            const float q = res[i] / norm;
            out[(size_t)gy * W + gx + i] = (va < q) ? q : va; // d_filter_gaussian.cu:84-87
        }
    }
}

// INTMAP (the frame pipeline's call): the maps hold integer-valued disparities whose differences stay inside the colour LUT --
// WTA writes d - zd, region voting bin - zd, so any two values differ by at most D - 1 = ncolor - 1.  The kernel is bound by
// vector-instruction issue (95 M wave instructions, every one 4 cycles: profiles/r03_pmc_sq_aggm.txt), 13 per pixel pair and tap,
// of which 8 only produce the LUT address (subtract, |.| -> int, clamp, shift, twice).  With a second tile holding 4 x (value +
// bias) as integers the LUT's BYTE OFFSET is one v_sad_u32 per pixel (|4a - 4b| = 4 |a - b|, exact), no clamp needed; weights
// and both running sums are computed exactly as before from the float tile.  The per-stage filter_bilateral_1 (arbitrary
// floats) keeps the general form.
template <int R, bool INTMAP>
__global__ __launch_bounds__(SF_TX *SF_TY) void stm_k_bilateral_r(const float *__restrict__ in0, float *__restrict__ out0,
                                                                 const float *__restrict__ in1, float *__restrict__ out1,
                                                                 const float *__restrict__ spatial,
                                                                 const float *__restrict__ color, int H, int W, int ncolor,
                                                                 const float *__restrict__ one_tab, int zd)
{
    const float *__restrict__ in = blockIdx.z ? in1 : in0; // both views of a frame share the launch
    float *__restrict__ out = blockIdx.z ? out1 : out0;
    constexpr int KW = 2 * R + 1, NF = (KW + 3 + 3) / 4 * 4;
    constexpr int TW = (SF_TX * 4 + 2 * R + 3) / 4 * 4 + 4, TH = SF_TY + 2 * R;
    __shared__ float4 tile4[TH * TW / 4];
    __shared__ uint4 itile4[INTMAP ? TH * TW / 4 : 1];
    extern __shared__ float ck[]; // colour LUT, ncolor entries
    float *tile = (float *)tile4;
    uint32_t *itile = (uint32_t *)itile4;
    const int tid = threadIdx.y * SF_TX + threadIdx.x;
    const int x0 = blockIdx.x * SF_TX * 4, y0 = blockIdx.y * SF_TY;
    // INTMAP is a promise of the caller (whole numbers, any two within the colour LUT); the block checks it on its own tile while
    // loading it and takes the general form when it does not hold, so a producer that breaks the promise costs speed, not results
    __shared__ int s_rng[3]; // min, max, any value that is not a whole number of moderate size
    if (INTMAP) {
        if (tid == 0) { s_rng[0] = 0x7fffffff; s_rng[1] = -0x7fffffff; s_rng[2] = 0; }
        __syncthreads();
    }
    int mn = 0x7fffffff, mx = -0x7fffffff, bad = 0;
    for (int i = tid; i < TH * TW; i += SF_TX * SF_TY) {
        const int ty = i / TW, tx = i - ty * TW;
        const int gx = min(max(x0 + tx - R, 0), W - 1), gy = min(max(y0 + ty - R, 0), H - 1);
        const float t = in[(size_t)gy * W + gx];
        tile[i] = t;
        if (INTMAP) {
            const int ti = (int)t;
            itile[i] = (uint32_t)((ti + (1 << 20)) * 4);
            bad |= !((float)ti == t) || (uint32_t)(ti + (1 << 19)) >= (1u << 20); // NaN, infinities, fractions, |value| >= 2^19
            mn = min(mn, ti);
            mx = max(mx, ti);
        }
    }
    if (INTMAP) { // per wave first (DPP), then one LDS atomic each; values outside +- 2^19 are flagged, so the bias cannot wrap
        const uint32_t bmx = wave_max_u32((uint32_t)(min(max(mx, -(1 << 19)), 1 << 19) + (1 << 20)));
        const uint32_t bmn = ~wave_max_u32(~(uint32_t)(min(max(mn, -(1 << 19)), 1 << 19) + (1 << 20)));
        const bool anybad = __ballot(bad != 0) != 0;
        if ((tid & 63) == 0) {
            atomicMin(&s_rng[0], (int)bmn - (1 << 20));
            atomicMax(&s_rng[1], (int)bmx - (1 << 20));
            if (anybad) atomicOr(&s_rng[2], 1);
        }
    }
    for (int i = tid; i < ncolor; i += SF_TX * SF_TY) ck[i] = color[i];
    __syncthreads();
    const bool fast = INTMAP && s_rng[2] == 0 && s_rng[1] - s_rng[0] < ncolor; // block-uniform
    // ... and a tile (with its halo) that holds ONE value -- 75 % of the tiles of the synthetic frame's disparity maps, 15 % on real
    // content -- gives every pixel the same sequence of operations, hence the same result: one wave computes it, all store it
    const bool one_value = fast && s_rng[0] == s_rng[1];
    __shared__ float s_one;
    const int gx = x0 + threadIdx.x * 4, gy = y0 + threadIdx.y;
    if (!one_value && (gx >= W || gy >= H)) return;
    // The four pixels are kept as two float2 pairs: weight, norm and result updates are v_pk_mul_f32 / v_pk_add_f32
    // (two pixels per instruction, each component rounded exactly like the scalar operation it replaces).
    typedef float f2 __attribute__((ext_vector_type(2)));
    const uint32_t ck_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float *)ck; // the LUT's address inside LDS
    float va[4];
    uint32_t ia[4];
    f2 res[2] = {{0.f, 0.f}, {0.f, 0.f}}, norm[2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        va[i] = tile[(threadIdx.y + R) * TW + threadIdx.x * 4 + i + R];
        ia[i] = INTMAP ? itile[(threadIdx.y + R) * TW + threadIdx.x * 4 + i + R] : 0u;
    }
    auto taps = [&](auto fast_) {
    constexpr bool FAST = decltype(fast_)::value;
    for (int y = 0; y < KW; ++y) {
        float row[NF];
        uint32_t irow[NF];
        const float4 *src = (const float4 *)(tile + (threadIdx.y + y) * TW + threadIdx.x * 4);
        const uint4 *isrc = (const uint4 *)(itile + (threadIdx.y + y) * TW + threadIdx.x * 4);
#pragma unroll
        for (int j = 0; j < NF / 4; ++j) {
            const float4 t = src[j];
            row[4 * j] = t.x; row[4 * j + 1] = t.y; row[4 * j + 2] = t.z; row[4 * j + 3] = t.w;
            if (FAST) {
                const uint4 u = isrc[j];
                irow[4 * j] = u.x; irow[4 * j + 1] = u.y; irow[4 * j + 2] = u.z; irow[4 * j + 3] = u.w;
            }
        }
        const float *krow = spatial + y * KW;
#pragma unroll
        for (int x = 0; x < KW; ++x) {
            const float gs = krow[x];
            const f2 gs2 = {gs, gs};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f2 vs = {row[x + 2 * h], row[x + 2 * h + 1]};
                f2 gc;
                if (FAST) {
                    // LDS byte addresses of the LUT entries: ck + 4 |a - b|, the table's own address riding in v_sad_u32's
                    // accumulate operand (round 3 added it with a separate v_add per pixel and tap: 60 of ~310 vector
                    // instructions per tile row)
                    typedef __attribute__((address_space(3))) const float lds_cf;
                    uint32_t b0, b1;
                    asm("v_sad_u32 %0, %1, %2, %3" : "=v"(b0) : "v"(ia[2 * h]), "v"(irow[x + 2 * h]), "s"(ck_lds));
                    asm("v_sad_u32 %0, %1, %2, %3" : "=v"(b1) : "v"(ia[2 * h + 1]), "v"(irow[x + 2 * h + 1]), "s"(ck_lds));
                    gc = f2{*(lds_cf *)(uintptr_t)b0, *(lds_cf *)(uintptr_t)b1};
                } else {
                    int c0 = (int)fabsf(va[2 * h] - vs.x), c1 = (int)fabsf(va[2 * h + 1] - vs.y); // d_filter_bilateral.cu:295
                    c0 = min(c0, ncolor - 1);
                    c1 = min(c1, ncolor - 1);
                    gc = f2{ck[c0], ck[c1]};
                }
                const f2 w = gs2 * gc;
                norm[h] = norm[h] + w;
                const f2 t = vs * w;
                res[h] = res[h] + t;
            }
        }
    }
    };
    if (one_value) {
        const int ci = s_rng[0] + zd; // the caller's table of results for one-value neighbourhoods (bilateral_one_value_table), or one wave's work
        if (one_tab != nullptr && ci >= 0 && ci < ncolor) {
            if (tid == 0) s_one = one_tab[ci];
        } else if (tid < 64) {
            taps(std::true_type());
            if (tid == 0) s_one = res[0].x / norm[0].x;
        }
        __syncthreads();
        if (gx >= W || gy >= H) return;
        const float r = s_one;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (gx + i < W) out[(size_t)gy * W + gx + i] = r;
        return;
    }
    if (INTMAP && fast) taps(std::true_type());
    else taps(std::false_type());
    const float r4[4] = {res[0].x, res[0].y, res[1].x, res[1].y}, n4[4] = {norm[0].x, norm[0].y, norm[1].x, norm[1].y};
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (gx + i < W) out[(size_t)gy * W + gx + i] = r4[i] / n4[i];
}

// sum of the weights in tap order, float32, exactly as every pixel's `norm = norm + weight` chain computes it
static float stencil_norm(int radius, float sigma)
{
    const int kw = 2 * radius + 1;
    std::vector<float> k((size_t)kw * kw);
    gaussian_kernel_2d(k.data(), radius, sigma);
    volatile float n = 0.0f;
    for (int i = 0; i < kw * kw; ++i) n = n + k[i];
    return n;
}

// ------------------------------------------------------------------ stencils
constexpr int ST_TX = 64, ST_TY = 4;

// bilateral: w = Gs[dx,dy] * Gc[(int)|v0 - v|], out = sum(w v) / sum(w)   (d_filter_bilateral.cu:278-303)
__global__ __launch_bounds__(ST_TX *ST_TY) void stm_k_bilateral(const float *__restrict__ in, float *__restrict__ out,
                                                               const float *__restrict__ spatial,
                                                               const float *__restrict__ color, int radius, int H, int W,
                                                               int ncolor)
{
    extern __shared__ float sm[];
    const int tw = ST_TX + 2 * radius, th = ST_TY + 2 * radius, kw = 2 * radius + 1;
    float *tile = sm, *sk = sm + tw * th, *ck = sk + kw * kw;
    int tid = threadIdx.y * ST_TX + threadIdx.x;
    int x0 = blockIdx.x * ST_TX, y0 = blockIdx.y * ST_TY;
    for (int i = tid; i < tw * th; i += ST_TX * ST_TY) {
        int ty = i / tw, tx = i - ty * tw;
        int gx = min(max(x0 + tx - radius, 0), W - 1), gy = min(max(y0 + ty - radius, 0), H - 1);
        tile[i] = in[(size_t)gy * W + gx];
    }
    for (int i = tid; i < kw * kw; i += ST_TX * ST_TY) sk[i] = spatial[i];
    for (int i = tid; i < ncolor; i += ST_TX * ST_TY) ck[i] = color[i];
    __syncthreads();
    int gx = x0 + threadIdx.x, gy = y0 + threadIdx.y;
    if (gx >= W || gy >= H) return;
    float va = tile[(threadIdx.y + radius) * tw + threadIdx.x + radius];
    float norm = 0.0f, res = 0.0f;
    for (int y = 0; y < kw; ++y) {
        const float *trow = tile + (threadIdx.y + y) * tw + threadIdx.x;
        const float *krow = sk + y * kw;
        for (int x = 0; x < kw; ++x) {
            float vs = trow[x];
            int ci = (int)fabsf(va - vs);
            ci = min(ci, ncolor - 1);
            float w = krow[x] * ck[ci];
            norm = norm + w;
            float t = vs * w;
            res = res + t;
        }
    }
    out[(size_t)gy * W + gx] = res / norm;
}

// the frame pipeline's two maps (left, right) in one launch of the radius-7 kernel
void launch_bilateral2(const float *in_a, float *out_a, const float *in_b, float *out_b, const float *spatial, const float *color,
                       int radius, int H, int W, int D, bool integer_maps, const float *one_value, int zd)
{
    if (radius != 7) {
        launch_bilateral(in_a, out_a, spatial, color, radius, H, W, D);
        launch_bilateral(in_b, out_b, spatial, color, radius, H, W, D);
        return;
    }
    ProfScope p("bilateral");
    if (integer_maps)
        STM_LAUNCH((stm_k_bilateral_r<7, true>), dim3(cdiv(W, SF_TX * 4), cdiv(H, SF_TY), 2), dim3(SF_TX, SF_TY), (size_t)D * 4, stream(), in_a, out_a,
                   in_b, out_b, spatial, color, H, W, D, one_value, zd);
    else
        STM_LAUNCH((stm_k_bilateral_r<7, false>), dim3(cdiv(W, SF_TX * 4), cdiv(H, SF_TY), 2), dim3(SF_TX, SF_TY), (size_t)D * 4, stream(), in_a, out_a,
                   in_b, out_b, spatial, color, H, W, D, (const float *)nullptr, 0);
    STM_CHECK_LAUNCH();
}

void launch_bilateral(const float *in, float *out, const float *spatial, const float *color, int radius, int H, int W,
                      int D)
{
    if (radius == 7) {
        ProfScope p("bilateral");
        if ((agg_variant() / 100) % 10 == 5) // 500 (tests): the frame pipeline's integer-map kernel on the caller's map; it checks every tile and
                                             // takes the general form where the map is not what it was promised
            STM_LAUNCH((stm_k_bilateral_r<7, true>), dim3(cdiv(W, SF_TX * 4), cdiv(H, SF_TY)), dim3(SF_TX, SF_TY), (size_t)D * 4, stream(),
                               in, out, in, out, spatial, color, H, W, D, (const float *)nullptr, 0);
        else
            STM_LAUNCH((stm_k_bilateral_r<7, false>), dim3(cdiv(W, SF_TX * 4), cdiv(H, SF_TY)), dim3(SF_TX, SF_TY), (size_t)D * 4, stream(),
                               in, out, in, out, spatial, color, H, W, D, (const float *)nullptr, 0);
        STM_CHECK_LAUNCH();
        return;
    }
    int tw = ST_TX + 2 * radius, th = ST_TY + 2 * radius, kw = 2 * radius + 1;
    size_t smem = (size_t)(tw * th + kw * kw + D) * 4;
    ProfScope p("bilateral");
    STM_LAUNCH(stm_k_bilateral, dim3(cdiv(W, ST_TX), cdiv(H, ST_TY)), dim3(ST_TX, ST_TY), smem, stream(), in, out,
                       spatial, color, radius, H, W, D);
    STM_CHECK_LAUNCH();
}

// grow-only gaussian: out = max(in, blur(in)); INVERT fuses op_invertnormf (x -> 1 - x) into the tile load
__global__ __launch_bounds__(ST_TX *ST_TY) void stm_k_gaussian_max(const float *__restrict__ in, float *__restrict__ out,
                                                                  const float *__restrict__ spatial, int radius, int H,
                                                                  int W, int invert)
{
    extern __shared__ float sm[];
    const int tw = ST_TX + 2 * radius, th = ST_TY + 2 * radius, kw = 2 * radius + 1;
    float *tile = sm, *sk = sm + tw * th;
    int tid = threadIdx.y * ST_TX + threadIdx.x;
    int x0 = blockIdx.x * ST_TX, y0 = blockIdx.y * ST_TY;
    for (int i = tid; i < tw * th; i += ST_TX * ST_TY) {
        int ty = i / tw, tx = i - ty * tw;
        int gx = min(max(x0 + tx - radius, 0), W - 1), gy = min(max(y0 + ty - radius, 0), H - 1);
        float v = in[(size_t)gy * W + gx];
        tile[i] = invert ? 1.0f - v : v;
    }
    for (int i = tid; i < kw * kw; i += ST_TX * ST_TY) sk[i] = spatial[i];
    __syncthreads();
    int gx = x0 + threadIdx.x, gy = y0 + threadIdx.y;
    if (gx >= W || gy >= H) return;
    float va = tile[(threadIdx.y + radius) * tw + threadIdx.x + radius];
    float norm = 0.0f, res = 0.0f;
    for (int y = 0; y < kw; ++y) {
        const float *trow = tile + (threadIdx.y + y) * tw + threadIdx.x;
        const float *krow = sk + y * kw;
        for (int x = 0; x < kw; ++x) {
            float w = krow[x];
            norm = norm + w;
            float t = trow[x] * w;
            res = res + t;
        }
    }
    float q = res / norm;
    out[(size_t)gy * W + gx] = (va < q) ? q : va; // d_filter_gaussian.cu:84-87
}

void launch_gaussian_max(const float *in, float *out, const float *spatial, int radius, float sigma, int H, int W,
                         bool invert_input)
{
    if (radius == 10 || radius == 7) {
        static std::map<std::pair<int, float>, float> norms;
        static std::mutex norms_mu; // first frames of two host threads may arrive together
        float norm;
        {
            std::lock_guard<std::mutex> lock(norms_mu);
            auto key = std::make_pair(radius, sigma);
            auto it = norms.find(key);
            if (it == norms.end()) it = norms.emplace(key, stencil_norm(radius, sigma)).first;
            norm = it->second;
        }
        ProfScope p("gaussian_max");
        if (radius == 10)
            STM_LAUNCH(stm_k_gaussian_max_r<10>, dim3(cdiv(W, SF_TX * 4), cdiv(H, SF_TY)), dim3(SF_TX, SF_TY), 0, stream(), in,
                               out, spatial, norm, H, W, invert_input ? 1 : 0);
        else
            STM_LAUNCH(stm_k_gaussian_max_r<7>, dim3(cdiv(W, SF_TX * 4), cdiv(H, SF_TY)), dim3(SF_TX, SF_TY), 0, stream(), in,
                               out, spatial, norm, H, W, invert_input ? 1 : 0);
        STM_CHECK_LAUNCH();
        return;
    }
    int tw = ST_TX + 2 * radius, th = ST_TY + 2 * radius, kw = 2 * radius + 1;
    size_t smem = (size_t)(tw * th + kw * kw) * 4;
    ProfScope p("gaussian_max");
    STM_LAUNCH(stm_k_gaussian_max, dim3(cdiv(W, ST_TX), cdiv(H, ST_TY)), dim3(ST_TX, ST_TY), smem, stream(), in, out,
                       spatial, radius, H, W, invert_input ? 1 : 0);
    STM_CHECK_LAUNCH();
}

} // namespace stm
