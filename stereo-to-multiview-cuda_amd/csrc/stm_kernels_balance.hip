// stm_kernels_balance.hip -- colour balance between the eyes (stm_set_balance, stm_balance_fit, stm_balance_apply; include/stm_hip.h
// has the definition line by line).  An addition, the reference has nothing like it: it takes graded studio masters.  Three kernels:
//   stm_k_balance_hist   both eyes' three channels into six 256-bin histograms, read straight from the caller's input (BGR or NV12,
//                        any packing): counted in LDS, the touched bins merged into 1536 global words with integer atomics;
//   stm_k_balance_fit    one workgroup, a thread per (channel, level): cumulative counts, the mid-rank match by binary search, the
//                        count-weighted smoothing from prefix sums, the carry, the limits, the running maximum, the state's update;
//   stm_k_balance_frame  the tables applied: the unpacked, converted pair written as one side-by-side BGR frame, the left half copied,
//                        which the plain frame path then takes.  With one image it is the stage stm_d_balance_apply.
// Integer arithmetic throughout, so nothing depends on the order anything ran in.  Nothing is read back: the state stays in device
// memory (as the depth budget's and the alignment's), so a frame stream's captured graphs replay the measurement.
#include "stm_common.h"
#include "stm_fetch.h"
#include <string.h>

namespace stm {

namespace {

constexpr int BL_BINS = 6 * 256; // hist[(e * 3 + c) * 256 + v]
constexpr int BL_RADIUS = 8;     // the smoothing window, fixed

// ---------------------------------------------------------------- step 1: the histograms
// One count per valid lane into the block's LDS histogram (stm_kernels_depth.hip's hist_add).  Real frames have flat regions -- sky,
// black bars, a letterboxed eye: 64 adds to one LDS address serialise, so up to BL_ROUNDS times the first pending lane's level is
// broadcast and every lane holding the same level is counted by that lane's single add; what is still pending after that adds for
// itself.  The loop is uniform for the wave (`todo` is a ballot).  Two rounds: a flat region and the edge of one.
constexpr int BL_ROUNDS = 2;
__device__ __forceinline__ void bal_hist_add(uint32_t *__restrict__ h, int b, bool valid)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid);
#pragma unroll 1
    for (int r = 0; r < BL_ROUNDS && todo; ++r) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __shfl(b, leader);
        const unsigned long long same = __ballot(valid && b == lb) & todo;
        if (lane == leader) atomicAdd(&h[lb], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&h[b], 1u);
}

__global__ __launch_bounds__(256) void stm_k_balance_hist_clear(uint32_t *__restrict__ hist)
{
    hist[blockIdx.x * 256 + threadIdx.x] = 0; // BL_BINS / 256 blocks
}

// Every pixel of both eyes counted once: a block walks whole 256-pixel tiles of the unpacked eye in row-major order (the trip count
// is uniform for the block, the last tile's tail lanes take no part).  n = H * W < 2^31.
template <int FMT, int AXIS, int FILT>
__global__ __launch_bounds__(256) void stm_k_balance_hist(uint32_t *__restrict__ hist, AlignSrc s, int W, uint32_t n)
{
    __shared__ uint32_t h[BL_BINS];
    for (int i = threadIdx.x; i < BL_BINS; i += 256) h[i] = 0;
    __syncthreads();
    const uint32_t step = gridDim.x * 256u; // <= 2^18, so base + step stays below 2^32
    for (uint32_t base = blockIdx.x * 256u; base < n; base += step) {
        const uint32_t i = base + threadIdx.x;
        const bool valid = i < n;
        const int y = valid ? (int)(i / (uint32_t)W) : 0, x = valid ? (int)(i % (uint32_t)W) : 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const uint32_t px = al_unpacked_px<FMT, AXIS, FILT>(s, e, y, x);
#pragma unroll
            for (int c = 0; c < 3; ++c) bal_hist_add(h + (e * 3 + c) * 256, (int)((px >> (8 * c)) & 0xff), valid);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BL_BINS; i += 256) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

// ---------------------------------------------------------------- steps 2 - 6: the fit
// 768 threads: thread (c, v) owns level v of channel c; every scan runs over the 256 threads of a channel, the three channels side
// by side, so every barrier is reached by all.  An inclusive Hillis-Steele scan of buf[0 .. 255] (this channel's row) in place.
template <class T, class Op> __device__ __forceinline__ T bal_scan(T *buf, int v, T x, Op op)
{
    buf[v] = x;
    __syncthreads();
#pragma unroll 1
    for (int d = 1; d < 256; d <<= 1) {
        T y = buf[v];
        if (v >= d) y = op(buf[v - d], y);
        __syncthreads();
        buf[v] = y;
        __syncthreads();
    }
    return buf[v];
}
struct BalAdd {
    template <class T> __device__ T operator()(T a, T b) const { return a + b; }
};
struct BalMax {
    template <class T> __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};

__global__ __launch_bounds__(768) void stm_k_balance_fit(int *__restrict__ state, const uint32_t *__restrict__ hist, int max_shift, int rate_q,
                                                         int fresh)
{
    __shared__ long long s_c0[3][256], s_c1[3][256], s_p[3][256];
    __shared__ int s_s[3][256], s_i[3][256], s_first[3];
    const int c = threadIdx.x >> 8, v = threadIdx.x & 255;
    const bool start = fresh || state[0] == 0; // read before any thread writes the state (the barriers below lie between)
    if (v == 0) s_first[c] = 256;
    // step 2: the cumulative counts of both eyes
    const long long h1 = (long long)hist[(3 + c) * 256 + v];
    const long long c0 = bal_scan(s_c0[c], v, (long long)hist[c * 256 + v], BalAdd());
    const long long c1 = bal_scan(s_c1[c], v, h1, BalAdd());
    (void)c0;
    // step 3: the mid-rank match, m = min{u : 2 C0[u] >= 2 C1[v] - h1[v]}; u = 255 always satisfies it
    const long long target = 2 * c1 - h1;
    int lo = 0, hi = 255;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (2 * s_c0[c][mid] >= target) hi = mid; else lo = mid + 1;
    }
    // step 4: the offsets, weighted by the right eye's counts over +-8 levels: window sums from prefix sums
    const long long off = (long long)(lo - v);
    bal_scan(s_p[c], v, h1 * off, BalAdd());
    const int w0 = max(v - BL_RADIUS, 0), w1 = min(v + BL_RADIUS, 255);
    const long long den = s_c1[c][w1] - (w0 > 0 ? s_c1[c][w0 - 1] : 0ll);
    const long long num = s_p[c][w1] - (w0 > 0 ? s_p[c][w0 - 1] : 0ll);
    int s = 0;
    if (den > 0) {
        const long long a = 2 * num + den, b = 2 * den;
        long long q = a / b; // C truncates: one less where a negative numerator leaves a remainder
        if (a % b < 0) --q;
        s = (int)q;
        atomicMin(&s_first[c], v);
    }
    s_s[c][v] = s;
    // ... an empty window takes the nearest level below that has one, else the nearest above
    const int j = bal_scan(s_i[c], v, den > 0 ? v : -1, BalMax()); // (its barriers publish s_s and s_first)
    s = s_s[c][j >= 0 ? j : min(s_first[c], 255)]; // (N >= 1: a window with counts exists)
    // step 5: the limits and the order
    s = min(max(s, -max_shift), max_shift);
    int t = min(max(v + s, 0), 255);
    t = bal_scan(s_i[c], v, t, BalMax());
    // step 6: the state, levels in 1/256
    const int x = 256 * t;
    int *st = state + 1 + threadIdx.x;
    if (start) {
        *st = x;
    } else {
        const int old = *st;
        *st = old + (int)(((long long)rate_q * ((long long)x - old) + 128) >> 8);
    }
    if (threadIdx.x == 0) state[0] = 1;
}

// ---------------------------------------------------------------- step 7: apply
// A block owns 256 columns of BL_ROWS output rows: columns [0, first_right) are the left eye, copied; the rest the right eye through
// the tables, which the block first puts into LDS -- from the state with step 7's rounding and clamp, or from the kernel argument.
// The stage call has first_right = 0 and one image as eye 1.
struct BalanceLut {
    u8 v[768];
};
constexpr int BL_ROWS = 16;
template <int FMT, int AXIS, int FILT>
__global__ __launch_bounds__(256) void stm_k_balance_frame(u8 *__restrict__ out, AlignSrc s, BalanceLut arg, const int *__restrict__ state, int H,
                                                           int first_right, int out_cols)
{
    __shared__ u8 lut[768];
    for (int i = threadIdx.x; i < 768; i += 256)
        lut[i] = state ? (u8)min(max((state[1 + i] + 128) >> 8, 0), 255) : arg.v[i];
    __syncthreads();
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= out_cols) return;
    const int y1 = min((int)(blockIdx.y + 1) * BL_ROWS, H);
    for (int y = blockIdx.y * BL_ROWS; y < y1; ++y) {
        uint32_t b, g, r;
        if (x < first_right) {
            const uint32_t px = al_unpacked_px<FMT, AXIS, FILT>(s, 0, y, x);
            b = px & 0xff; g = (px >> 8) & 0xff; r = (px >> 16) & 0xff;
        } else {
            const uint32_t px = al_unpacked_px<FMT, AXIS, FILT>(s, 1, y, x - first_right);
            b = lut[px & 0xff]; g = lut[256 + ((px >> 8) & 0xff)]; r = lut[512 + ((px >> 16) & 0xff)];
        }
        u8 *d = out + ((size_t)y * out_cols + x) * s.elem_sz;
        d[0] = (u8)b; d[1] = (u8)g; d[2] = (u8)r;
    }
}

struct HistLaunch {
    uint32_t *hist;
    AlignSrc s;
    int H, W;
    template <int FMT, int AXIS, int FILT> void run() const
    {
        const uint32_t n = (uint32_t)((size_t)H * W);
        const unsigned blocks = n / 256 >= 1024 ? 1024u : (n + 255) / 256;
        STM_LAUNCH((stm_k_balance_hist<FMT, AXIS, FILT>), dim3(blocks), dim3(256), 0, stream(), hist, s, W, n);
    }
};
struct BalanceFrameLaunch {
    u8 *out;
    AlignSrc s;
    BalanceLut lut;
    const int *state;
    int H, first_right, out_cols;
    template <int FMT, int AXIS, int FILT> void run() const
    {
        STM_LAUNCH((stm_k_balance_frame<FMT, AXIS, FILT>), dim3(cdiv(out_cols, 256), cdiv(H, BL_ROWS)), dim3(256), 0, stream(), out, s, lut, state,
                   H, first_right, out_cols);
    }
};

} // namespace

void launch_balance_measure(int *state, uint32_t *hist, const PackInput *in, const u8 *img_l, const u8 *img_r, int H, int W, int elem_sz,
                            int max_shift, int rate_q, bool fresh)
{
    {
        ProfScope p("balance_hist");
        STM_LAUNCH(stm_k_balance_hist_clear, dim3(BL_BINS / 256), dim3(256), 0, stream(), hist); // a kernel, not a memset node
        dispatch(in, HistLaunch{hist, make_src(in, img_l, img_r, H, W, elem_sz), H, W});
        STM_CHECK_LAUNCH();
    }
    ProfScope p("balance_fit");
    STM_LAUNCH(stm_k_balance_fit, dim3(1), dim3(768), 0, stream(), state, hist, max_shift, rate_q, fresh ? 1 : 0);
    STM_CHECK_LAUNCH();
}

void launch_balance_frame(u8 *out, const PackInput *in, const u8 *img, int H, int W, int elem_sz, const u8 *lut768, const int *state)
{
    ProfScope p("balance_frame");
    BalanceLut lut;
    if (lut768) memcpy(lut.v, lut768, 768); else memset(lut.v, 0, 768);
    dispatch(in, BalanceFrameLaunch{out, make_src(in, img, img, H, W, elem_sz), lut, state, H, in ? W : 0, in ? 2 * W : W});
    STM_CHECK_LAUNCH();
}

} // namespace stm
