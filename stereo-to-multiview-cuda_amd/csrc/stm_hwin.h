// stm_hwin.h -- the horizontal window table of stm_k_pq_hsr (stm_kernels_aggh.hip): record layout and the routine that builds
// the records of the four 16-pixel tiles a wave's 64 lanes cover.  Shared by the stand-alone table kernel and stm_k_cross_arms,
// which has the arms in registers when it finishes (one pass over the arm planes and one launch less per frame).
#pragma once
#include "stm_common.h"

namespace stm {

constexpr int HR_TOP = 36;  // a tile's sweep range starts this many pixels left of the tile: pixels [16 t - 36, 16 t + 52)
constexpr int HR_NG = 22;   // groups of four pixels in that range
constexpr int HR_REC = 64;  // dwords per table record: [0] first group of the sweep inside the range, [1] its groups n, [8 + 2 p ..] mask of the group that block p of
                            // the kernel's 22 sweep blocks handles (the sweep is blocks 22 - n .. 21)

template <int N> __device__ __forceinline__ int hr_row_ror(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x120 + N, 0xf, 0xf, false); }

template <int N> __device__ __forceinline__ uint32_t hr_row_shr(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + N, 0xf, 0xf, false); }

// One record per DPP row of 16 lanes.  Lane m of the row owns the window [s0, s0 + nn) (nn = 0: none) along the walk's axis,
// R0 (a multiple of 4) is the first step of the tile's range, every window lies inside [R0, R0 + 88).  A window toggles its
// lane's bit at its first step and at the step after its last; the running XOR over the steps gives every step's set of
// lanes, and four consecutive steps are one group's 64-bit mask.  ev: 96 dwords of LDS owned by this row of lanes.  dst: the
// record, or nullptr (nothing is stored).
static __device__ __forceinline__ void win16_build(uint32_t *__restrict__ dst, uint32_t *ev, int R0, int s0, int nn)
{
    const int m = threadIdx.x & 15;
    int lo = nn ? s0 : 0x7fffffff, hi = nn ? s0 + nn : -0x7fffffff; // over the tile's 16 lanes; every lane gets the result
    lo = min(lo, hr_row_ror<8>(lo)); lo = min(lo, hr_row_ror<4>(lo)); lo = min(lo, hr_row_ror<2>(lo)); lo = min(lo, hr_row_ror<1>(lo));
    hi = max(hi, hr_row_ror<8>(hi)); hi = max(hi, hr_row_ror<4>(hi)); hi = max(hi, hr_row_ror<2>(hi)); hi = max(hi, hr_row_ror<1>(hi));
    const int K0 = hi > lo ? (lo & ~3) : 0, n = hi > lo ? (hi - K0 + 3) >> 2 : 0; // n <= 22
    const int q0 = n ? (K0 - R0) >> 2 : 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) ev[6 * m + i] = 0u;
    __builtin_amdgcn_wave_barrier();
    if (nn) {
        atomicXor(&ev[s0 - K0], 1u << m);
        atomicXor(&ev[s0 + nn - K0], 1u << m);
    }
    __builtin_amdgcn_wave_barrier();
    // lane m scans steps 6 m .. 6 m + 5, then the lanes' totals are scanned along the row
    uint32_t e[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) e[i] = ev[6 * m + i];
#pragma unroll
    for (int i = 1; i < 6; ++i) e[i] ^= e[i - 1];
    uint32_t tot = e[5];
    tot ^= hr_row_shr<1>(tot); tot ^= hr_row_shr<2>(tot); tot ^= hr_row_shr<4>(tot); tot ^= hr_row_shr<8>(tot);
    const uint32_t before = hr_row_shr<1>(tot); // XOR of all steps in front of this lane's six
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 6; ++i) ev[6 * m + i] = e[i] ^ before; // the step's set of lanes
    __builtin_amdgcn_wave_barrier();
    if (!dst) return;
    if (m < 2) dst[m] = m == 0 ? (uint32_t)q0 : (uint32_t)n;
#pragma unroll
    for (int j = m; j < HR_NG; j += 16)
        if (j < n) {
            const unsigned long long mk = (unsigned long long)ev[4 * j] | ((unsigned long long)ev[4 * j + 1] << 16) |
                                          ((unsigned long long)ev[4 * j + 2] << 32) | ((unsigned long long)ev[4 * j + 3] << 48);
            *(unsigned long long *)(dst + 8 + 2 * (HR_NG - n + j)) = mk; // the sweep's last group in slot 21
        }
}

// lane l of the wave = pixel x0 + l of image row y (x0 a multiple of 64), aL / aR its horizontal arms (any value for x >= W).
// A DPP row of 16 lanes per tile: lane 16 r + m = pixel m of the wave's r-th tile, whose window is [x - armL, x + armR)
// (d_ca_cross_sum.cu:277-289).  ev4: 4 x 96 dwords of LDS owned by this wave.  `tab`: records of this view.
static __device__ __forceinline__ void hwin_build(uint32_t *__restrict__ tab, uint32_t *ev4, int y, int x0, int aL, int aR, int W, int nTx)
{
    const int l = threadIdx.x & 63, r = l >> 4;
    const int x = x0 + l, t = x >> 4;
    int s0 = 0, nn = 0;
    if (x < W) { // (a tile past the row: no windows, nothing is stored)
        s0 = x - aL;
        nn = aL + aR;
    }
    win16_build(t < nTx ? tab + ((size_t)y * nTx + t) * HR_REC : nullptr, ev4 + r * 96, 16 * t - HR_TOP, s0, nn);
}

// The vertical twin (stm_k_pq_v12m, stm_kernels_aggv.hip: one column per wave): the same record per (tile of 16 rows, column),
// the walk's axis being y.  Lane 16 c + m = row 16 u + m of column x0 + c, s0 / nn its window [y - armU, y + armD) (nn = 0: none;
// d_ca_cross_sum.cu:172-173,189-194): mask bit 16 a + m of a group = row m has the group's row a in its window.
// `tile`: the records of (view, tile u), column x at + x * HR_REC; every column in [x0, x0 + 4) must exist there.
static __device__ __forceinline__ void vcol_build(uint32_t *__restrict__ tile, uint32_t *ev4, int u, int x0, int s0, int nn)
{
    const int r = (threadIdx.x & 63) >> 4;
    win16_build(tile + (size_t)(x0 + r) * HR_REC, ev4 + r * 96, 16 * u - HR_TOP, s0, nn);
}

// ---- the arms of a column as jump offsets (stm_k_pq_v12r, stm_kernels_aggv.hip: exact window sums as runs of vector adds).
// One dword per (view, column, row): [view][column][VA_PAD + y], va_rows(H) rows per column (the kernel reads a step ahead and a
// pass behind without clamping; only rows of the image are ever used).  The kernel keeps the last VA_RING rows of either pass in
// registers, row r of its input in slot (r - VA_LAG) mod VA_RING, row r of the first pass in slot r mod VA_RING, and holds, per
// ring, one sequence of VA_RING adds for every slot a window can end in: sequence e adds the slots e + 1 .. e + VA_RING (mod
// VA_RING) in that order, VA_SEQ bytes each (the adds and the return).  The window [y - armU, y + armD) of L rows ends in row
// y + armD - 1, that is in sequence e = (y + armD - 1 - VA_LAG) mod VA_RING of the input ring, and is summed by entering that
// sequence L adds before its end: the entry is that byte offset.  The second pass uses the same offset in the other ring's
// sequences, which are laid out VA_LAG slots further on.  L = 0 enters at the return.
constexpr int VA_RING = 72;             // rows per ring: 2 usd at the largest usd the kernel takes
constexpr int VA_LAG = 36;              // the second pass runs this many rows behind the first
constexpr int VA_SEQ = 4 * VA_RING + 4; // bytes of a sequence
constexpr int VA_PAD = 72;              // table rows in front of row 0
static inline __host__ __device__ int va_rows(int H) { return H + 128; }
static inline __host__ __device__ uint32_t va_entry(int y, int aU, int aD)
{
    int L = aU + aD;
    L = L > VA_RING ? VA_RING : L;
    const int e = (y + aD - 1 - VA_LAG + 2 * VA_RING) % VA_RING; // (y + aD - 1 >= 0 - 1)
    return (uint32_t)(VA_SEQ * e + 4 * (VA_RING - L));
}

// ---- the vertical window table (stm_k_vwin_table, stm_kernels_aggm.hip; layout: DESIGN.md section 3) -- one record, one wave.
// Lane l = (column b = l / 16 of the group, row i = l % 16 of the tile); s0 / nn = first row and length of the lane's window
// [y - armU, y + armD) (nn = 0: no window).  ev: VT_EV (or, top >= 0: 96) 64-bit slots of LDS owned by this wave.
// top >= 0: the static layout of stm_k_pq_v12r ([0] first quad of the sweep inside the tile's range, masks of range quad J at 8 + 8 J).
__device__ __forceinline__ int hw_wave_min_i(int v)
{
    v = min(v, hr_row_ror<8>(v)); v = min(v, hr_row_ror<4>(v)); v = min(v, hr_row_ror<2>(v)); v = min(v, hr_row_ror<1>(v));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ int hw_wave_max_i(int v)
{
    v = max(v, hr_row_ror<8>(v)); v = max(v, hr_row_ror<4>(v)); v = max(v, hr_row_ror<2>(v)); v = max(v, hr_row_ror<1>(v));
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
static __device__ __forceinline__ void vwin_build(uint32_t *__restrict__ dst, unsigned long long *ev, int u, int top, int s0, int nn)
{
    const int l = threadIdx.x & 63;
    const int lo = hw_wave_min_i(nn ? s0 : 0x7fffffff);
    const int hi = hw_wave_max_i(nn ? s0 + nn : -0x7fffffff);
    const int K0 = hi > lo ? (lo & ~3) : 0, n_it = hi > lo ? (hi - K0 + 3) >> 2 : 0;
    const int q0 = top >= 0 && n_it ? (K0 - (16 * u - top)) >> 2 : 0;
    if (l < 8) dst[l] = l == 0 ? (uint32_t)(top >= 0 ? q0 : K0) : l == 1 ? (uint32_t)n_it : 0u;
    unsigned long long *mk = (unsigned long long *)(dst + 8) + 4 * q0;
    const int steps = 4 * n_it;
    for (int j = l; j <= steps; j += 64) ev[j] = 0ull;
    __builtin_amdgcn_wave_barrier();
    if (nn) { // the window [s0, s0 + nn) lies inside [K0, K0 + steps]
        atomicXor(&ev[s0 - K0], 1ull << l);
        atomicXor(&ev[s0 + nn - K0], 1ull << l);
    }
    __builtin_amdgcn_wave_barrier();
    unsigned long long carry = 0ull;
    for (int base = 0; base < steps; base += 64) {
        unsigned long long e = base + l < steps ? ev[base + l] : 0ull;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(e, o);
            if (l >= o) e ^= t;
        }
        e ^= carry;
        if (base + l < steps) mk[base + l] = e;
        carry = __shfl(e, 63);
    }
}

} // namespace stm
