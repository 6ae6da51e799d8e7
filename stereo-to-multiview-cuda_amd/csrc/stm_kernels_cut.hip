// stm_kernels_cut.hip -- shot changes detected on the device (stm_set_cut, stm_cut_detect; include/stm_hip.h has the definition line
// by line).  An addition, the reference has nothing like it: it has no state that outlives a frame.  Three launches:
//   stm_k_cut_sig_clear  the 256 scratch words of the signature;
//   stm_k_cut_sig        the left eye's signature, read straight from the caller's input (BGR or NV12, any packing): a 16-bin
//                        luma histogram in each cell of a 4 x 4 grid, counted in LDS, the touched bins merged into 256 global
//                        words with integer atomics;
//   stm_k_cut_decide     one workgroup, a thread per word: the L1 distance to the stored signature, the score, the decision, the
//                        new state, and on a cut one 32-bit zero into the `valid` word of up to three recursive states.
// Integer arithmetic throughout, so nothing depends on the order anything ran in.  Nothing is read back: the state stays in device
// memory (as the states it resets), so a frame stream's captured graphs replay the detector.
#include "stm_common.h"
#include "stm_fetch.h"

namespace stm {

namespace {

constexpr int CUT_BINS = 256; // sig[cell * 16 + bin]

// ---------------------------------------------------------------- step 1: the signature
// One count per valid lane into the block's LDS histogram: stm_kernels_balance.hip's bal_hist_add (a copy: that file's and the
// depth fit's stay where they are), on the combined index cell * 16 + bin.  A wave's 64 consecutive pixels mostly lie in one cell
// and in a few bins, so up to CUT_ROUNDS times the first pending lane's index is broadcast and every lane holding the same index is
// counted by that lane's single add; what is still pending after that adds for itself.  The loop is uniform for the wave (`todo`
// is a ballot).
constexpr int CUT_ROUNDS = 2;
__device__ __forceinline__ void cut_hist_add(uint32_t *__restrict__ h, int b, bool valid)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid);
#pragma unroll 1
    for (int r = 0; r < CUT_ROUNDS && todo; ++r) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __shfl(b, leader);
        const unsigned long long same = __ballot(valid && b == lb) & todo;
        if (lane == leader) atomicAdd(&h[lb], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&h[b], 1u);
}

__global__ __launch_bounds__(256) void stm_k_cut_sig_clear(uint32_t *__restrict__ sig)
{
    sig[threadIdx.x] = 0;
}

// Every pixel of the left eye counted once: a block walks whole 256-pixel tiles of the unpacked eye in row-major order (the trip
// count is uniform for the block, the last tile's tail lanes take no part).  n = H * W < 2^31, H, W >= 4; 4 y and 4 x stay below 2^31.
template <int FMT, int AXIS, int FILT>
__global__ __launch_bounds__(256) void stm_k_cut_sig(uint32_t *__restrict__ sig, AlignSrc s, int H, int W, uint32_t n)
{
    __shared__ uint32_t h[CUT_BINS];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t step = gridDim.x * 256u; // <= 2^18, so base + step stays below 2^32
    for (uint32_t base = blockIdx.x * 256u; base < n; base += step) {
        const uint32_t i = base + threadIdx.x;
        const bool valid = i < n;
        const int y = valid ? (int)(i / (uint32_t)W) : 0, x = valid ? (int)(i % (uint32_t)W) : 0;
        const uint32_t px = al_unpacked_px<FMT, AXIS, FILT>(s, 0, y, x);
        const uint32_t Y = ((px & 0xff) + 2 * ((px >> 8) & 0xff) + ((px >> 16) & 0xff)) >> 2;
        const uint32_t cell = (4u * (uint32_t)y / (uint32_t)H) * 4u + 4u * (uint32_t)x / (uint32_t)W;
        cut_hist_add(h, (int)(cell * 16u + (Y >> 4)), valid);
    }
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    if (c) atomicAdd(&sig[threadIdx.x], c);
}

// ---------------------------------------------------------------- steps 2 - 4: the score, the decision, the resets
// 256 threads, thread i owns word i of the signature.  Both sums (|diff| and the old signature) are reduced inside each of the four
// waves with shuffles and across them through LDS; thread 0 decides.  Every read of the old state lies before the barrier, every
// write after it.
__device__ __forceinline__ long long cut_wave_sum(long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;
}

__global__ __launch_bounds__(256) void stm_k_cut_decide(int *__restrict__ state, const uint32_t *__restrict__ sig, uint32_t n,
                                                        int thresh_permille, int min_gap, uint32_t *reset0, uint32_t *reset1,
                                                        uint32_t *reset2)
{
    __shared__ long long s_d[4], s_o[4];
    const int i = threadIdx.x;
    const long long cur = (long long)sig[i], old = (long long)(uint32_t)state[4 + i];
    const int old_valid = state[0], old_since = state[2];
    const long long d = cut_wave_sum(cur > old ? cur - old : old - cur), o = cut_wave_sum(old);
    if ((i & 63) == 0) {
        s_d[i >> 6] = d;
        s_o[i >> 6] = o;
    }
    __syncthreads();
    state[4 + i] = (int)sig[i]; // stored on every frame, on a suppressed cut as well
    if (i != 0) return;
    const long long D = s_d[0] + s_d[1] + s_d[2] + s_d[3], O = s_o[0] + s_o[1] + s_o[2] + s_o[3];
    const bool history = old_valid != 0 && O == (long long)n; // a state left by a frame of another size: no history
    const int score = history ? (int)((1000ll * D) / (2ll * (long long)n)) : 1000;
    const long long s1 = (long long)old_since + 1;
    const int since = (int)(s1 < (1ll << 30) ? s1 : (1ll << 30));
    const bool cut = !history || (score >= thresh_permille && since >= min_gap);
    state[0] = 1;
    state[1] = cut ? 1 : 0;
    state[2] = cut ? 0 : since;
    state[3] = score;
    if (cut) { // zero is the `valid` word of a float state and of an int state alike
        if (reset0) *reset0 = 0u;
        if (reset1) *reset1 = 0u;
        if (reset2) *reset2 = 0u;
    }
}

struct SigLaunch {
    uint32_t *sig;
    AlignSrc s;
    int H, W;
    template <int FMT, int AXIS, int FILT> void run() const
    {
        const uint32_t n = (uint32_t)((size_t)H * W);
        const unsigned blocks = n / 256 >= 1024 ? 1024u : (n + 255) / 256;
        STM_LAUNCH((stm_k_cut_sig<FMT, AXIS, FILT>), dim3(blocks), dim3(256), 0, stream(), sig, s, H, W, n);
    }
};

} // namespace

void launch_cut_detect(int *state, uint32_t *sig, const PackInput *in, const u8 *img_l, int H, int W, int elem_sz, int thresh_permille,
                       int min_gap, void *reset0, void *reset1, void *reset2)
{
    {
        ProfScope p("cut_sig");
        STM_LAUNCH(stm_k_cut_sig_clear, dim3(1), dim3(256), 0, stream(), sig); // a kernel, not a memset node
        dispatch(in, SigLaunch{sig, make_src(in, img_l, img_l, H, W, elem_sz), H, W});
        STM_CHECK_LAUNCH();
    }
    ProfScope p("cut_decide");
    STM_LAUNCH(stm_k_cut_decide, dim3(1), dim3(256), 0, stream(), state, (const uint32_t *)sig, (uint32_t)((size_t)H * W), thresh_permille,
               min_gap, (uint32_t *)reset0, (uint32_t *)reset1, (uint32_t *)reset2);
    STM_CHECK_LAUNCH();
}

} // namespace stm
