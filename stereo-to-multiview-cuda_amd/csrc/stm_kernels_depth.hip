// stm_kernels_depth.hip -- the measurement behind the automatic depth budget (stm_set_depth mode 2, stm_depth_fit; stm_hip.h).
//
// An addition, the reference has nothing like it: its N views always span the camera baseline.  Two kernels:
//   stm_k_disp_hist   both disparity maps into one histogram of 4096 quarter-pixel bins;
//   stm_k_depth_fit   one wave: the clipped range [d_lo, d_hi] from the histogram, the gain and convergence that bring it into the
//                     budget, and the update of the four-float state the renderer of the same frame reads.
// Nothing is read back: the state stays in device memory, so a frame stream's captured graphs replay the fit.
#include "stm_common.h"

namespace stm {

constexpr int DH_BINS = 4096;

// v = disp * 4; clamped to [-2048, 2047] (C fmaxf: a NaN becomes -2048, bin 0); rounded half up
__device__ __forceinline__ int depth_bin(float disp)
{
    float v = disp * 4.0f;
    v = fminf(fmaxf(v, -2048.0f), 2047.0f);
    return (int)floorf(v + 0.5f) + 2048; // 0 .. 4095
}

// One count per valid lane into the block's LDS histogram.  Real maps are dominated by a few values (the zero-parallax plane, the
// background): 64 adds to one LDS address serialise, so up to DH_ROUNDS times the first pending lane's bin is broadcast and every
// lane holding the same bin is counted by that lane's single add; what is still pending after that adds for itself.  The loop is
// uniform for the wave (`todo` is a ballot).
constexpr int DH_ROUNDS = 4;
__device__ __forceinline__ void hist_add(uint32_t *__restrict__ h, int b, bool valid)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid);
#pragma unroll 1
    for (int r = 0; r < DH_ROUNDS && todo; ++r) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __shfl(b, leader);
        const unsigned long long same = __ballot(valid && b == lb) & todo;
        if (lane == leader) atomicAdd(&h[lb], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&h[b], 1u);
}

__global__ __launch_bounds__(256) void stm_k_disp_hist_clear(uint32_t *__restrict__ hist)
{
    hist[blockIdx.x * 256 + threadIdx.x] = 0; // DH_BINS / 256 blocks
}

// Every pixel of both maps counted once: a block walks whole 256-pixel tiles (the trip count is uniform for the block, the last
// tile's tail lanes take no part), counts into its 16 KB LDS histogram and merges the bins it touched into `hist` with integer
// atomics -- the result does not depend on the order anything ran in.
__global__ __launch_bounds__(256) void stm_k_disp_hist(uint32_t *__restrict__ hist, const float *__restrict__ disp_l,
                                                       const float *__restrict__ disp_r, size_t n)
{
    __shared__ uint32_t h[DH_BINS];
    for (int i = threadIdx.x; i < DH_BINS; i += 256) h[i] = 0;
    __syncthreads();
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t base = (size_t)blockIdx.x * 256; base < n; base += step) {
        const size_t i = base + threadIdx.x;
        const bool valid = i < n;
        const int bl = valid ? depth_bin(disp_l[i]) : 0;
        const int br = valid ? depth_bin(disp_r[i]) : 0;
        hist_add(h, bl, valid);
        hist_add(h, br, valid);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DH_BINS; i += 256) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

// The same count over the pixels of both maps inside the active rectangle only (stm_depth_fit_rect): `rect` holds {top, bottom, left,
// right} in device memory, clamped to the map here, and the rectangle is walked as one run of rh * rw pixels (its rows keep the
// map's pitch, so the lanes run along x).  The grid was sized on the host from the whole map, an upper bound: a block whose first
// tile lies past the run's end does nothing.  H W < 2^31 (screened).
__global__ __launch_bounds__(256) void stm_k_disp_hist_rect(uint32_t *__restrict__ hist, const float *__restrict__ disp_l,
                                                            const float *__restrict__ disp_r, int H, int W, const int *__restrict__ rect)
{
    __shared__ uint32_t h[DH_BINS];
    const int t = min(max(rect[0], 0), H), b = min(max(rect[1], t), H), l = min(max(rect[2], 0), W), r = min(max(rect[3], l), W);
    const uint32_t rw = (uint32_t)(r - l), n = (uint32_t)(b - t) * rw;
    if (blockIdx.x * 256u >= n) return; // uniform for the block; an empty rectangle counts nothing
    for (int i = threadIdx.x; i < DH_BINS; i += 256) h[i] = 0;
    __syncthreads();
    const uint32_t step = gridDim.x * 256u; // <= 2^18 and base < 2^31: no wrap
    for (uint32_t base = blockIdx.x * 256u; base < n; base += step) {
        const uint32_t i = base + threadIdx.x;
        const bool valid = i < n;
        const uint32_t y = valid ? i / rw : 0u, x = valid ? i - y * rw : 0u;
        const size_t at = (size_t)(t + (int)y) * W + (size_t)(l + (int)x);
        const int bl = valid ? depth_bin(disp_l[at]) : 0;
        const int br = valid ? depth_bin(disp_r[at]) : 0;
        hist_add(h, bl, valid);
        hist_add(h, br, valid);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DH_BINS; i += 256) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

struct DepthFitArgs {
    float disp_lo, disp_hi, max_gain, rate;
    int clip_permille;
    int fresh; // the state's history is ignored (a null d_state: every frame fitted on its own)
};

// One wave.  Lane l owns bins 64 l .. 64 l + 63: its sum, an inclusive scan over the lanes, then the one lane whose range holds
// the crossing walks its 64 bins.  lo = the smallest b with cum(b) > k; hi = the largest b whose suffix count is > k.
__global__ __launch_bounds__(64) void stm_k_depth_fit(float *__restrict__ state, const uint32_t *__restrict__ hist, DepthFitArgs p)
{
    __shared__ uint32_t h[DH_BINS];
    __shared__ int s_lo, s_hi;
    const int lane = threadIdx.x;
    for (int i = lane; i < DH_BINS; i += 64) h[i] = hist[i];
    if (lane == 0) { s_lo = 0; s_hi = DH_BINS - 1; }
    __syncthreads();
    uint32_t own = 0;
    for (int j = 0; j < 64; ++j) own += h[lane * 64 + ((j + lane) & 63)]; // rotated: the lanes hit 64 different banks
    uint32_t incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    const uint32_t total = __shfl(incl, 63); // n = 2 H W
    const uint32_t excl = incl - own;
    const unsigned long long k = (unsigned long long)total * (unsigned long long)p.clip_permille / 1000ull;
    // lo: the first lane whose inclusive count exceeds k (total > k, so there is one)
    const unsigned long long m_lo = __ballot((unsigned long long)incl > k);
    // hi: the last lane whose suffix count (its own bins and everything above) exceeds k
    const unsigned long long m_hi = __ballot((unsigned long long)(total - excl) > k);
    if (m_lo && lane == __ffsll((long long)m_lo) - 1) {
        unsigned long long cum = excl;
        int b = lane * 64;
        for (int j = 0; j < 64; ++j) {
            cum += h[lane * 64 + j];
            if (cum > k) { b = lane * 64 + j; break; }
        }
        s_lo = b;
    }
    if (m_hi && lane == 63 - __clzll((long long)m_hi)) {
        unsigned long long suf = total - incl;
        int b = lane * 64 + 63;
        for (int j = 63; j >= 0; --j) {
            suf += h[lane * 64 + j];
            if (suf > k) { b = lane * 64 + j; break; }
        }
        s_hi = b;
    }
    __syncthreads();
    if (lane != 0) return;
    const float d_lo = (float)(s_lo - 2048) * 0.25f;
    const float d_hi = (float)(s_hi - 2048) * 0.25f;
    // the fit, in double, one operation per line (the file is compiled -ffp-contract=off; the f64 division is the correctly rounded one)
    const double span = (double)d_hi - (double)d_lo;
    const double budget = (double)p.disp_hi - (double)p.disp_lo;
    double g = span > 0.0 ? budget / span : (double)p.max_gain;
    g = fmin(g, (double)p.max_gain);
    double a = g * (double)d_hi;
    a = a - (double)p.disp_hi; // the least conv that brings the far end in
    double b = g * (double)d_lo;
    b = b - (double)p.disp_lo; // the most conv that keeps the near end in
    const double c = fmin(fmax(0.0, a), b);
    if (p.fresh || state[0] == 0.0f) {
        state[0] = 1.0f;
        state[1] = (float)g;
        state[2] = (float)c;
        state[3] = 0.0f;
        return;
    }
    const double og = (double)state[1], oc = (double)state[2];
    double t = g - og;
    t = (double)p.rate * t;
    state[1] = (float)(og + t);
    t = c - oc;
    t = (double)p.rate * t;
    state[2] = (float)(oc + t);
}

// hist: DH_BINS words of scratch; state: four floats {valid, gain, conv, 0}; d_rect: the active rectangle's four words in device
// memory, or null: the whole maps, with the launches as they always were
void launch_depth_fit(float *state, uint32_t *hist, const float *disp_l, const float *disp_r, int H, int W, float disp_lo, float disp_hi,
                      float max_gain, int clip_permille, float rate, bool fresh, const int *d_rect)
{
    const size_t n = (size_t)H * W;
    const int blocks = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    {
        ProfScope p("disp_hist");
        STM_LAUNCH(stm_k_disp_hist_clear, dim3(DH_BINS / 256), dim3(256), 0, stream(), hist); // a kernel, not a memset node
        if (d_rect) STM_LAUNCH(stm_k_disp_hist_rect, dim3(blocks), dim3(256), 0, stream(), hist, disp_l, disp_r, H, W, d_rect);
        else STM_LAUNCH(stm_k_disp_hist, dim3(blocks), dim3(256), 0, stream(), hist, disp_l, disp_r, n);
        STM_CHECK_LAUNCH();
    }
    ProfScope p("depth_fit");
    const DepthFitArgs a{disp_lo, disp_hi, max_gain, rate, clip_permille, fresh ? 1 : 0};
    STM_LAUNCH(stm_k_depth_fit, dim3(1), dim3(64), 0, stream(), state, hist, a);
    STM_CHECK_LAUNCH();
}

} // namespace stm
