// stm_kernels_active.hip -- the active picture area found on the device (stm_set_active, stm_active_detect, stm_active_fill;
// include/stm_hip.h has the definition line by line), for gfx950.  An addition, the reference has nothing like it: it matches and
// measures black bars as if they were picture.  Three launches measure:
//   stm_k_active_clear   the H + W scratch words of the counts;
//   stm_k_active_count   the left eye's lit pixels per row and per column, read straight from the caller's input (BGR or NV12, any
//                        packing): a block owns 64 columns by ACT_ROWS rows, a lane is a column, a wave walks rows;
//   stm_k_active_decide  one workgroup: the first and last picture row and column, the bars of this frame, the hold rule and the
//                        new state of 16 ints.
// and one applies:
//   stm_k_active_fill    every map pixel outside the rectangle becomes one value; only the four strips are visited.
// (stm_k_active_rect writes a given rectangle's four words where the consumers read them.)
// Integer arithmetic throughout, so nothing depends on the order anything ran in.  Nothing is read back: state and rectangle stay in
// device memory, so a frame stream's captured graphs replay the measurement and everything that reads it.
#include "stm_common.h"
#include "stm_fetch.h"

namespace stm {

namespace {

constexpr int ACT_COLS = 64; // a tile's columns: one per lane
constexpr int ACT_ROWS = 64; // a tile's rows: 16 per wave of the block's four

__global__ __launch_bounds__(256) void stm_k_active_clear(uint32_t *__restrict__ counts, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x; // n = H + W <= 2^31, the grid covers it once
    if (i < n) counts[i] = 0;
}

// counts[y] = the lit pixels of row y, counts[H + x] = the lit pixels of column x.  A row's share of a tile is the popcount of the
// wave's ballot: one add per wave and row, none where the tile's part of the row is dark.  A column's share is summed in the lane's
// register over the wave's rows, across the block's four waves through LDS, then one add per column and block, none where it is 0.
// So a row word takes at most ceil(W / 64) adds and a column word at most ceil(H / 64), and the bars themselves take none.
template <int FMT, int AXIS, int FILT>
__global__ __launch_bounds__(256) void stm_k_active_count(uint32_t *__restrict__ counts, AlignSrc s, int H, int W, int tiles_x, int thresh_luma)
{
    __shared__ uint32_t col[4][ACT_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ty = (int)(blockIdx.x / (uint32_t)tiles_x), tx = (int)(blockIdx.x % (uint32_t)tiles_x);
    const long long xl = (long long)tx * ACT_COLS + lane; // < W + 64, which need not fit an int: compared in 64 bits
    const bool in_x = xl < (long long)W;
    const int x = in_x ? (int)xl : 0;
    const long long y0 = (long long)ty * ACT_ROWS + wave * (ACT_ROWS / 4);
    uint32_t mine = 0;
#pragma unroll 1
    for (int r = 0; r < ACT_ROWS / 4; ++r) {
        const long long yl = y0 + r;
        if (yl >= (long long)H) break; // uniform for the wave
        const int y = (int)yl;
        bool lit = false;
        if (in_x) {
            const uint32_t px = al_unpacked_px<FMT, AXIS, FILT>(s, 0, y, x);
            const uint32_t Y = ((px & 0xff) + 2 * ((px >> 8) & 0xff) + ((px >> 16) & 0xff)) >> 2;
            lit = (int)Y > thresh_luma;
        }
        const unsigned long long m = __ballot(lit);
        if (lane == 0 && m) atomicAdd(&counts[y], (uint32_t)__popcll(m));
        mine += lit ? 1u : 0u;
    }
    col[wave][lane] = mine;
    __syncthreads();
    if (wave != 0 || !in_x) return;
    const uint32_t c = col[0][lane] + col[1][lane] + col[2][lane] + col[3][lane];
    if (c) atomicAdd(&counts[(size_t)H + x], c);
}

struct CountLaunch {
    uint32_t *counts;
    AlignSrc s;
    int H, W, thresh_luma;
    template <int FMT, int AXIS, int FILT> void run() const
    {
        const long long tx = ((long long)W + ACT_COLS - 1) / ACT_COLS, ty = ((long long)H + ACT_ROWS - 1) / ACT_ROWS; // tx * ty <= H W / 4096 + H / 64 + W / 64 + 1 < 2^31
        STM_LAUNCH((stm_k_active_count<FMT, AXIS, FILT>), dim3((unsigned)(tx * ty)), dim3(256), 0, stream(), counts, s, H, W, (int)tx, thresh_luma);
    }
};

struct ActiveArgs {
    int H, W, lit_permille, max_bar_permille, hold, restart;
    const int *cut_state; // the shot-change detector's state or null: word 1 is this frame's cut flag
};

// The first and the last picture line of n lines: every thread keeps the least and greatest index it saw over its stride, a wave
// reduces with shuffles, the block through LDS.  None: first = n, last = -1.
__device__ __forceinline__ void active_span(const uint32_t *__restrict__ cnt, int n, unsigned long long rhs, int (*part)[2], int *first, int *last)
{
    int lo = n, hi = -1;
    for (int i = threadIdx.x; i < n; i += 256) {
        if ((unsigned long long)cnt[i] * 1000ull > rhs) {
            lo = min(lo, i);
            hi = max(hi, i);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min(lo, __shfl_xor(lo, d));
        hi = max(hi, __shfl_xor(hi, d));
    }
    __syncthreads(); // `part` may still be read from the call before
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = lo;
        part[threadIdx.x >> 6][1] = hi;
    }
    __syncthreads();
    *first = min(min(part[0][0], part[1][0]), min(part[2][0], part[3][0]));
    *last = max(max(part[0][1], part[1][1]), max(part[2][1], part[3][1]));
}

// Steps 3 to 7 of the definition.  Every read of the old state lies before the barrier, every write after it; thread 0 decides.
__global__ __launch_bounds__(256) void stm_k_active_decide(int *__restrict__ state, const uint32_t *__restrict__ counts, ActiveArgs p)
{
    __shared__ int part[4][2];
    __shared__ int old[16];
    if (threadIdx.x < 16) old[threadIdx.x] = state[threadIdx.x];
    const bool cut = p.cut_state && p.cut_state[1] == 1;
    int r0, r1, c0, c1;
    active_span(counts, p.H, (unsigned long long)p.lit_permille * (unsigned long long)p.W, part, &r0, &r1);
    active_span(counts + p.H, p.W, (unsigned long long)p.lit_permille * (unsigned long long)p.H, part, &c0, &c1);
    __syncthreads(); // `old` is complete (the spans' barriers already say so: this one says it here)
    if (threadIdx.x != 0) return;
    const int H = p.H, W = p.W;
    const bool history = old[0] != 0 && old[6] == H && old[7] == W;
    const bool restart = !history || p.restart != 0 || cut;
    if (r1 < 0 || c1 < 0) { // blank
        if (!restart) {
            state[5] = 0; // a fade through black says nothing
            return;
        }
        const int blank[16] = {0, 0, H, 0, W, 0, H, W, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 16; ++i) state[i] = blank[i];
        return;
    }
    const int cap_y = (int)((long long)H * p.max_bar_permille / 1000), cap_x = (int)((long long)W * p.max_bar_permille / 1000);
    const int m[4] = {min(r0, cap_y), min(H - 1 - r1, cap_y), min(c0, cap_x), min(W - 1 - c1, cap_x)};
    // the rectangle the bars are compared with: the state's with history, the whole frame without
    const int was[4] = {history ? old[1] : 0, history ? old[2] : H, history ? old[3] : 0, history ? old[4] : W};
    int B[4] = {was[0], H - was[1], was[2], W - was[3]}, cand[4], run[4];
    for (int i = 0; i < 4; ++i) {
        cand[i] = old[8 + i];
        run[i] = old[12 + i];
        const int b = m[i];
        if (restart) {
            B[i] = b; cand[i] = b; run[i] = 0;
        } else if (b < B[i]) { // picture inside the bar: given back at once
            B[i] = b; run[i] = 0;
        } else if (b == B[i]) {
            run[i] = 0;
        } else {
            cand[i] = run[i] == 0 ? b : min(cand[i], b);
            run[i] += 1;
            if (run[i] >= p.hold) { B[i] = cand[i]; run[i] = 0; }
        }
    }
    const int now[4] = {B[0], H - B[1], B[2], W - B[3]};
    const int changed = (now[0] != was[0] || now[1] != was[1] || now[2] != was[2] || now[3] != was[3]) ? 1 : 0;
    state[0] = 1;
    for (int i = 0; i < 4; ++i) state[1 + i] = now[i];
    state[5] = changed;
    state[6] = H;
    state[7] = W;
    for (int i = 0; i < 4; ++i) { state[8 + i] = cand[i]; state[12 + i] = run[i]; }
}

__global__ __launch_bounds__(64) void stm_k_active_rect(int *__restrict__ d_rect, int top, int bottom, int left, int right)
{
    if (threadIdx.x == 0) { d_rect[0] = top; d_rect[1] = bottom; d_rect[2] = left; d_rect[3] = right; }
}

struct FillArgs {
    float *disp[2];
    int nmaps, H, W;
    const int *rect;
    float value;
};

// The pixels outside the rectangle as one run: the rows above it, the rows below it, then per rectangle row the columns left and
// right of it.  The grid was sized on the host from the whole map -- an upper bound, the rectangle is known on the device only --
// and a block whose first tile lies past the run's end does nothing: a full rectangle writes nothing.  The four words are clamped
// to the map first, so whatever they hold no store leaves it.
__global__ __launch_bounds__(256) void stm_k_active_fill(FillArgs a)
{
    const long long H = a.H, W = a.W;
    const long long t = min(max((long long)a.rect[0], 0ll), H), b = min(max((long long)a.rect[1], t), H);
    const long long l = min(max((long long)a.rect[2], 0ll), W), r = min(max((long long)a.rect[3], l), W);
    const long long n_top = t * W, n_bot = (H - b) * W, side = l + (W - r), n = n_top + n_bot + (b - t) * side;
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        long long y, x;
        if (i < n_top) {
            y = i / W; x = i - y * W;
        } else if (i < n_top + n_bot) {
            const long long j = i - n_top;
            y = b + j / W; x = j - (j / W) * W;
        } else {
            const long long j = i - n_top - n_bot, q = j / side, k = j - q * side;
            y = t + q; x = k < l ? k : r + (k - l);
        }
        const size_t at = (size_t)(y * W + x);
        a.disp[0][at] = a.value;
        if (a.nmaps > 1) a.disp[1][at] = a.value;
    }
}

} // namespace

void launch_active_detect(int *state, uint32_t *counts, const PackInput *in, const u8 *img_l, int H, int W, int elem_sz, int thresh_luma,
                          int lit_permille, int max_bar_permille, int hold, bool restart, const int *cut_state)
{
    {
        ProfScope p("active_clear");
        const uint32_t n = (uint32_t)H + (uint32_t)W;
        STM_LAUNCH(stm_k_active_clear, dim3((n + 255) / 256), dim3(256), 0, stream(), counts, n); // a kernel, not a memset node
    }
    {
        ProfScope p("active_count");
        dispatch(in, CountLaunch{counts, make_src(in, img_l, img_l, H, W, elem_sz), H, W, thresh_luma});
        STM_CHECK_LAUNCH();
    }
    ProfScope p("active_decide");
    const ActiveArgs a{H, W, lit_permille, max_bar_permille, hold, restart ? 1 : 0, cut_state};
    STM_LAUNCH(stm_k_active_decide, dim3(1), dim3(256), 0, stream(), state, (const uint32_t *)counts, a);
    STM_CHECK_LAUNCH();
}

void launch_active_rect(int *d_rect, const int rect[4])
{
    ProfScope p("active_rect");
    STM_LAUNCH(stm_k_active_rect, dim3(1), dim3(64), 0, stream(), d_rect, rect[0], rect[1], rect[2], rect[3]);
    STM_CHECK_LAUNCH();
}

void launch_active_fill(int nmaps, float *const *disp, int H, int W, const int *d_rect, float value)
{
    ProfScope p("active_fill");
    const size_t tiles = ((size_t)H * W + 255) / 256;
    const FillArgs a{{disp[0], nmaps > 1 ? disp[1] : nullptr}, nmaps, H, W, d_rect, value};
    STM_LAUNCH(stm_k_active_fill, dim3((unsigned)(tiles < 1024 ? tiles : 1024)), dim3(256), 0, stream(), a);
    STM_CHECK_LAUNCH();
}

} // namespace stm
