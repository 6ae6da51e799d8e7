// stm_kernels_ovfit.hip -- the measurement behind the overlay's automatic depth placement (stm_set_overlay_auto, stm_overlay_fit;
// stm_hip.h has the definition line by line), for gfx950.
//
// An addition, the reference has no overlay at all.  Four launches ahead of the compositor:
//   stm_k_ovfit_clear  the 4096 bins and the four words of the alpha box (a kernel, not a memset node: DESIGN section 4);
//   stm_k_ovfit_box    the least and greatest overlay row and column that hold a pixel with alpha != 0;
//   stm_k_ovfit_hist   both maps under the box's footprint into one histogram of 4096 quarter-pixel bins, NaNs left out;
//   stm_k_ovfit_fit    one wave: the near percentile, the budget's map, the margin and the limits, and the update of the four-float
//                      state {valid, disparity, nearest, 0} the compositor of the same frame reads.
// Nothing is read back: box, histogram and state stay in device memory, so a frame stream launches the four behind its captured
// graph with arguments that change from submit to submit.  Every sum is an integer one: no result depends on the order anything ran.
#include "stm_common.h"

#pragma clang fp contract(off) // the fit's f64 lines are one operation each (the Makefile's -ffp-contract=off says the same)

namespace stm {

namespace {
constexpr int OF_BINS = 4096;
constexpr int OF_EMPTY_LO = 0x7fffffff; // the box's least row / column while no pixel has been seen; the greatest starts at -1

// stm_depth_fit's binning line (stm_kernels_depth.hip, which stays as it is: DESIGN section 25): v = disp * 4 clamped to
// [-2048, 2047], rounded half up.  The caller leaves NaNs out
__device__ __forceinline__ int ovfit_bin(float disp)
{
    float v = disp * 4.0f;
    v = fminf(fmaxf(v, -2048.0f), 2047.0f);
    return (int)floorf(v + 0.5f) + 2048; // 0 .. 4095
}

// stm_k_disp_hist's aggregation of equal bins, copied: up to OF_ROUNDS times the first pending lane's bin is broadcast and every lane
// holding the same bin is counted by that lane's single add; what is still pending after that adds for itself.  Uniform for the wave
constexpr int OF_ROUNDS = 4;
__device__ __forceinline__ void ovfit_hist_add(uint32_t *__restrict__ h, int b, bool valid)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid);
#pragma unroll 1
    for (int r = 0; r < OF_ROUNDS && todo; ++r) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __shfl(b, leader);
        const unsigned long long same = __ballot(valid && b == lb) & todo;
        if (lane == leader) atomicAdd(&h[lb], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&h[b], 1u);
}

struct OvFitGeom {
    int ov_rows, ov_cols, x0, y0; // the overlay in view pixel space
    int Hv, Wv, H, W;             // the view and the maps
    int pad;
};
struct OvFitRect {
    int y0, y1, x0, x1; // map pixels, half open; empty: y0 >= y1 or x0 >= x1
};
// steps 1 and 2 of the definition from the four box words {r0, r1, q0, q1}: the footprint in view pixels, clipped, then in map
// pixels (floor at the near end, ceiling at the far end), in 64-bit integers
__device__ __forceinline__ OvFitRect ovfit_rect(const OvFitGeom &g, const int *__restrict__ box)
{
    OvFitRect r = {0, 0, 0, 0};
    const int r0 = box[0], r1 = box[1], q0 = box[2], q1 = box[3];
    if (r1 < r0 || q1 < q0) return r; // no pixel with alpha != 0
    long long ya = (long long)g.y0 + r0 - g.pad, yb = (long long)g.y0 + r1 + 1 + g.pad;
    long long xa = (long long)g.x0 + q0 - g.pad, xb = (long long)g.x0 + q1 + 1 + g.pad;
    ya = ya < 0 ? 0 : ya; yb = yb > g.Hv ? g.Hv : yb;
    xa = xa < 0 ? 0 : xa; xb = xb > g.Wv ? g.Wv : xb;
    if (ya >= yb || xa >= xb) return r;
    r.y0 = (int)(ya * g.H / g.Hv); r.y1 = (int)((yb * g.H + g.Hv - 1) / g.Hv);
    r.x0 = (int)(xa * g.W / g.Wv); r.x1 = (int)((xb * g.W + g.Wv - 1) / g.Wv);
    return r;
}
// the footprint's interval [a, b) of one axis moved into the active interval [A, B): their intersection where there is one, else as
// much of the footprint's length as fits, taken from the active end nearest to it (a subtitle that lies wholly in a bar is placed
// by the picture lines next to it)
__device__ __forceinline__ void ovfit_slide(int &a, int &b, int A, int B)
{
    const int lo = max(a, A), hi = min(b, B);
    if (lo < hi) { a = lo; b = hi; return; }
    const int len = min(b - a, B - A);
    if (b <= A) { a = A; b = A + len; }
    else { b = B; a = B - len; }
}
} // namespace

// ws: OF_BINS words of histogram, then the box {r0, r1, q0, q1}
// zero_state: four floats of scratch that stand in for a null d_state, or null
__global__ __launch_bounds__(256) void stm_k_ovfit_clear(uint32_t *__restrict__ ws, float *__restrict__ zero_state)
{
    ws[blockIdx.x * 256 + threadIdx.x] = 0; // OF_BINS / 256 blocks
    if (blockIdx.x == 0 && threadIdx.x < 4) {
        ((int *)ws)[OF_BINS + threadIdx.x] = (threadIdx.x & 1) ? -1 : OF_EMPTY_LO;
        if (zero_state) zero_state[threadIdx.x] = 0.0f;
    }
}

// An overlay pixel is read as a dword.  A block takes a chunk of OF_BOX_COLS columns (blockIdx.x) of the rows blockIdx.y,
// blockIdx.y + gridDim.y, ...; a thread keeps the least and greatest row and column with alpha != 0 it saw, the wave reduces them
// with shuffles, the block through LDS, and one thread sends at most four atomicMin / atomicMax -- none for a bound the box already
// holds (the words only ever move outwards, so a stale read can only cost a redundant atomic).  One atomic per wave, as first
// written, serialised on the four words: 1.5 ms for a full 1080p overlay.
constexpr int OF_BOX_COLS = 2048, OF_BOX_ROWS = 512;
__global__ __launch_bounds__(256) void stm_k_ovfit_box(int *__restrict__ box, const uint32_t *__restrict__ ov, int ov_rows, int ov_cols)
{
    __shared__ int part[4][4];
    const int c0 = (int)blockIdx.x * OF_BOX_COLS, c1 = min(c0 + OF_BOX_COLS, ov_cols);
    int rlo = OF_EMPTY_LO, rhi = -1, qlo = OF_EMPTY_LO, qhi = -1;
    for (int row = (int)blockIdx.y; row < ov_rows; row += (int)gridDim.y) {
        const uint32_t *__restrict__ line = ov + (size_t)row * ov_cols;
        for (int col = c0 + (int)threadIdx.x; col < c1; col += 256) {
            if ((line[col] >> 24) != 0) {
                rlo = min(rlo, row); rhi = max(rhi, row);
                qlo = min(qlo, col); qhi = max(qhi, col);
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        rlo = min(rlo, __shfl_xor(rlo, d));
        rhi = max(rhi, __shfl_xor(rhi, d));
        qlo = min(qlo, __shfl_xor(qlo, d));
        qhi = max(qhi, __shfl_xor(qhi, d));
    }
    if ((threadIdx.x & 63) == 0) {
        int *w = part[threadIdx.x >> 6];
        w[0] = rlo; w[1] = rhi; w[2] = qlo; w[3] = qhi;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int i = 1; i < 4; ++i) {
        rlo = min(rlo, part[i][0]); rhi = max(rhi, part[i][1]);
        qlo = min(qlo, part[i][2]); qhi = max(qhi, part[i][3]);
    }
    if (rhi < 0) return; // the block saw no pixel with alpha != 0
    const volatile int *now = box;
    if (rlo < now[0]) atomicMin(&box[0], rlo);
    if (rhi > now[1]) atomicMax(&box[1], rhi);
    if (qlo < now[2]) atomicMin(&box[2], qlo);
    if (qhi > now[3]) atomicMax(&box[3], qhi);
}

// Both maps inside the footprint's map rectangle, which every block derives from the box words: the rectangle is walked as one run
// of rh * rw pixels in 256-pixel tiles (its rows keep the map's pitch, so the lanes run along x), the grid was sized on the host
// from the overlay's full rectangle -- an upper bound -- and a block whose first tile lies past the end does nothing.  Counts go
// into the block's 16 KB LDS histogram; the bins it touched are merged with integer atomics.
// active != nullptr (stm_overlay_fit_rect): the map rectangle is first moved into the active one, per axis.
__device__ __forceinline__ void ovfit_hist_body(uint32_t *__restrict__ h, uint32_t *__restrict__ ws, const float *__restrict__ disp_l,
                                                const float *__restrict__ disp_r, const OvFitGeom &g, const int *__restrict__ active)
{
    OvFitRect rc = ovfit_rect(g, (const int *)ws + OF_BINS);
    if (active && rc.y0 < rc.y1 && rc.x0 < rc.x1) { // the four words clamped to the map first: whatever they hold, no load leaves it
        const int t = min(max(active[0], 0), g.H), b = min(max(active[1], t), g.H), l = min(max(active[2], 0), g.W), r = min(max(active[3], l), g.W);
        ovfit_slide(rc.y0, rc.y1, t, b);
        ovfit_slide(rc.x0, rc.x1, l, r);
    }
    if (rc.y0 >= rc.y1 || rc.x0 >= rc.x1) return; // uniform for the grid
    const uint32_t rw = (uint32_t)(rc.x1 - rc.x0);
    const uint32_t n = (uint32_t)(rc.y1 - rc.y0) * rw; // <= H W < 2^31 (screened)
    if (blockIdx.x * 256u >= n) return;                 // uniform for the block
    for (int i = threadIdx.x; i < OF_BINS; i += 256) h[i] = 0;
    __syncthreads();
    const uint32_t step = gridDim.x * 256u;
    for (uint32_t base = blockIdx.x * 256u; base < n; base += step) { // base < 2^31 and step <= 2^18: no wrap
        const uint32_t i = base + threadIdx.x;
        const bool in = i < n;
        const uint32_t y = in ? i / rw : 0u, x = in ? i - y * rw : 0u;
        const size_t at = (size_t)(rc.y0 + (int)y) * g.W + (size_t)(rc.x0 + (int)x);
        const float vl = in ? disp_l[at] : 0.0f, vr = in ? disp_r[at] : 0.0f;
        const bool okl = in && vl == vl, okr = in && vr == vr; // a NaN is not counted
        ovfit_hist_add(h, okl ? ovfit_bin(vl) : 0, okl);
        ovfit_hist_add(h, okr ? ovfit_bin(vr) : 0, okr);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < OF_BINS; i += 256) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&ws[i], c);
    }
}
__global__ __launch_bounds__(256) void stm_k_ovfit_hist(uint32_t *__restrict__ ws, const float *__restrict__ disp_l,
                                                        const float *__restrict__ disp_r, OvFitGeom g)
{
    __shared__ uint32_t h[OF_BINS];
    ovfit_hist_body(h, ws, disp_l, disp_r, g, nullptr);
}
__global__ __launch_bounds__(256) void stm_k_ovfit_hist_rect(uint32_t *__restrict__ ws, const float *__restrict__ disp_l,
                                                             const float *__restrict__ disp_r, OvFitGeom g, const int *__restrict__ active)
{
    __shared__ uint32_t h[OF_BINS];
    ovfit_hist_body(h, ws, disp_l, disp_r, g, active);
}

struct OvFitArgs {
    float gain, conv;          // the depth budget in force, unless depth_state != nullptr
    const float *depth_state;  // depth mode 2: gain and conv are state[1] and state[2], written earlier on the same stream
    const int *cut_state;      // the shot-change detector's state or null: word 1 is this frame's cut flag
    int near_permille;
    float margin, limit_lo, limit_hi, rate_near, rate_far;
    int Wv, W;
    int fresh; // restart, or a null d_state: the state's history is ignored
};

// One wave, the shape of stm_k_depth_fit.  Lane l owns bins 64 l .. 64 l + 63: its sum, an inclusive scan over the lanes, then the
// one lane whose range holds the crossing walks its 64 bins: lo = the smallest b with cum(b) > k.  Lane 0 does steps 4 to 6.
__global__ __launch_bounds__(64) void stm_k_ovfit_fit(float *__restrict__ state, const uint32_t *__restrict__ hist, OvFitArgs p)
{
    __shared__ uint32_t h[OF_BINS];
    __shared__ int s_lo;
    const int lane = threadIdx.x;
    for (int i = lane; i < OF_BINS; i += 64) h[i] = hist[i];
    if (lane == 0) s_lo = 0;
    __syncthreads();
    uint32_t own = 0;
    for (int j = 0; j < 64; ++j) own += h[lane * 64 + ((j + lane) & 63)]; // rotated: the lanes hit 64 different banks
    uint32_t incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    const uint32_t total = __shfl(incl, 63); // n <= 2 H W < 2^32
    if (total == 0) return;                  // n == 0: none of the four floats is written
    const uint32_t excl = incl - own;
    const unsigned long long k = (unsigned long long)total * (unsigned long long)p.near_permille / 1000ull;
    const unsigned long long m_lo = __ballot((unsigned long long)incl > k); // total > k, so there is one
    if (lane == __ffsll((long long)m_lo) - 1) {
        unsigned long long cum = excl;
        int b = lane * 64;
        for (int j = 0; j < 64; ++j) {
            cum += h[lane * 64 + j];
            if (cum > k) { b = lane * 64 + j; break; }
        }
        s_lo = b;
    }
    __syncthreads();
    if (lane != 0) return;
    const double dp = (double)(s_lo - 2048) * 0.25;
    const double g = (double)(p.depth_state ? p.depth_state[1] : p.gain), c = (double)(p.depth_state ? p.depth_state[2] : p.conv);
    // the target, in double, one operation per line (the f64 division is the correctly rounded one)
    double e = g * dp;
    e = e - c;
    e = e * (double)p.Wv;
    e = e / (double)p.W;
    double t = e - (double)p.margin;
    t = fmin(fmax(t, (double)p.limit_lo), (double)p.limit_hi);
    double d = t;
    const bool cut = p.cut_state && p.cut_state[1] == 1;
    if (!(p.fresh || cut || state[0] == 0.0f)) {
        const double od = (double)state[1];
        const double r = t < od ? (double)p.rate_near : (double)p.rate_far;
        double u = t - od;
        u = r * u;
        d = od + u;
        d = fmin(fmax(d, (double)p.limit_lo), (double)p.limit_hi);
    }
    state[0] = 1.0f;
    state[1] = (float)d;
    state[2] = (float)e;
    state[3] = 0.0f;
}

// ws: OVERLAY_FIT_WS_WORDS words of scratch; state: four floats {valid, disparity, nearest, 0}; zero_state: they are scratch and
// zeroed first (a null d_state: a fit that counts nothing leaves disparity 0); d_rect: the active rectangle's four words in device
// memory, or null: the footprint as it is, with the launches as they always were.  Screened by the caller
void launch_overlay_fit(float *state, uint32_t *ws, const float *disp_l, const float *disp_r, int H, int W, const u8 *ov, int ov_rows,
                        int ov_cols, int x0, int y0, int Hv, int Wv, float gain, float conv, const float *depth_state, const OverlayAuto &oa,
                        bool fresh, bool zero_state, const int *cut_state, const int *d_rect)
{
    {
        ProfScope p("ovfit_box");
        STM_LAUNCH(stm_k_ovfit_clear, dim3(OF_BINS / 256), dim3(256), 0, stream(), ws, zero_state ? state : nullptr);
        STM_LAUNCH(stm_k_ovfit_box, dim3(cdiv(ov_cols, OF_BOX_COLS), ov_rows < OF_BOX_ROWS ? ov_rows : OF_BOX_ROWS), dim3(256), 0, stream(), (int *)ws + OF_BINS, (const uint32_t *)ov, ov_rows,
                   ov_cols);
        STM_CHECK_LAUNCH();
    }
    const OvFitGeom g = {ov_rows, ov_cols, x0, y0, Hv, Wv, H, W, oa.pad};
    // the grid: the map rectangle of the overlay's FULL rectangle plus pad, which holds the alpha box's whatever the pixels are
    // (|x0|, |y0| <= 65536, sides <= 65535, pad <= 4096: the sums stay far inside 64 bits; the products are below 2^62)
    long long ya = (long long)y0 - oa.pad, yb = (long long)y0 + ov_rows + oa.pad, xa = (long long)x0 - oa.pad, xb = (long long)x0 + ov_cols + oa.pad;
    ya = ya < 0 ? 0 : ya; yb = yb > Hv ? Hv : yb;
    xa = xa < 0 ? 0 : xa; xb = xb > Wv ? Wv : xb;
    if (ya < yb && xa < xb) {
        const long long rows = (yb * H + Hv - 1) / Hv - ya * H / Hv, cols = (xb * W + Wv - 1) / Wv - xa * W / Wv;
        const long long tiles = (rows * cols + 255) / 256;
        ProfScope p("ovfit_hist");
        const dim3 grid((unsigned)(tiles < 1024 ? tiles : 1024)); // the slid rectangle is never larger than the footprint's
        if (d_rect) STM_LAUNCH(stm_k_ovfit_hist_rect, grid, dim3(256), 0, stream(), ws, disp_l, disp_r, g, d_rect);
        else STM_LAUNCH(stm_k_ovfit_hist, grid, dim3(256), 0, stream(), ws, disp_l, disp_r, g);
        STM_CHECK_LAUNCH();
    }
    ProfScope p("ovfit_fit");
    const OvFitArgs a{gain, conv, depth_state, cut_state, oa.near_permille, oa.margin, oa.limit_lo, oa.limit_hi, oa.rate_near, oa.rate_far, Wv, W,
                      fresh ? 1 : 0};
    STM_LAUNCH(stm_k_ovfit_fit, dim3(1), dim3(64), 0, stream(), state, ws, a);
    STM_CHECK_LAUNCH();
}

} // namespace stm
