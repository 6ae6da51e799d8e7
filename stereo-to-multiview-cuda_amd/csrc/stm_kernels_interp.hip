// stm_kernels_interp.hip -- outlier interpolation (Mei et al. 3.4, "proper interpolation", the step after region voting): every
// pixel the L/R check marked and region voting could not vote away takes the disparity of a reliable pixel found along one of 16
// directions.  An addition: the reference has no such step.
//
// Definition (include/stm_hip.h): a pixel is reliable iff outl == 0.  For every other pixel p, walk the 16
// directions of IP_DX / IP_DY in that order, visiting p + k (dx, dy), k = 1, 2, ..., until the position leaves the image; the first
// reliable pixel met is the direction's candidate.  outl[p] == 2 (occlusion): the candidate with the largest value, folded in
// direction order with "replace when v > best" (so NaN iff the first direction that has a candidate carries NaN).  Any other
// class (mismatch): the candidate whose colour is closest to p's (|dB| + |dG| + |dR|), ties to the earlier direction.  No
// candidate: p keeps its value.  Only outliers are written and only reliable pixels are read, so the step runs in place.
//
// One kernel, stm_k_interp, for one or two views (blockIdx.y).  The work is a sparse set of pixels (1 - 12 % of an image) with
// 16 independent walks each, so the lanes are not laid along x:
//   phase 1  a block takes IP_PX consecutive pixels (row-major) and compacts its outliers into an LDS list (ballot + prefix);
//   phase 2  one 16-lane row per outlier, one direction per lane, four outliers per wave; a lane fetches IP_U positions of its
//            walk per round trip (the loads are independent, the tests on them run in walk order);
//   phase 3  16-way arg-reduction inside the row with __shfl_xor(.., 16) over a total order that equals the sequential fold:
//            occlusion (value descending, direction ascending) over the non-NaN candidates unless the first candidate is NaN;
//            mismatch the integer key colour distance * 16 + direction, minimum.  Lane 0 of the row stores the winner's value.
#include "stm_common.h"

namespace stm {

constexpr int IP_T = 256;   // threads per block: 16 rows of 16 lanes
constexpr int IP_PX = 1024; // pixels a block compacts and serves
constexpr int IP_U = 4;     // positions of a walk fetched per round trip

// the 16 directions, (dx, dy) with y growing downwards; nibble j of the packed words = component + 2
constexpr int IP_DX[16] = {1, 2, 1, 1, 0, -1, -1, -2, -1, -2, -1, -1, 0, 1, 1, 2};
constexpr int IP_DY[16] = {0, 1, 1, 2, 1, 2, 1, 1, 0, -1, -1, -2, -1, -2, -1, -1};
constexpr unsigned long long ip_pack(const int *c, int j = 0) { return j == 16 ? 0ull : ((unsigned long long)(c[j] + 2) << (4 * j)) | ip_pack(c, j + 1); }
constexpr unsigned long long IP_DX_NIB = ip_pack(IP_DX), IP_DY_NIB = ip_pack(IP_DY);

struct InterpArgs { // both views of a frame share the launch
    float *disp[2];
    const u8 *outl[2], *img[2];
};

__global__ __launch_bounds__(IP_T) void stm_k_interp(InterpArgs a, int H, int W, int elem_sz)
{
    __shared__ uint32_t s_list[IP_PX]; // pixel indices of the block's outliers (any order: the pixels are independent)
    __shared__ uint32_t s_n;
    const int v = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    float *disp = a.disp[v]; // read where outl == 0, written where outl != 0
    const u8 *__restrict__ outl = a.outl[v];
    const u8 *__restrict__ img = a.img[v];
    const uint32_t HW = (uint32_t)H * (uint32_t)W, p0 = blockIdx.x * (uint32_t)IP_PX;

    // ---- phase 1: the block's outliers
    if (tid == 0) s_n = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < IP_PX / IP_T; ++k) {
        const uint32_t p = p0 + k * IP_T + tid;
        const bool o = p < HW && outl[p] != 0;
        const unsigned long long m = __ballot(o);
        uint32_t base = 0;
        if (lane == 0 && m) base = atomicAdd(&s_n, (uint32_t)__popcll(m));
        base = __shfl(base, 0);
        if (o) s_list[base + __popcll(m & ((1ull << lane) - 1ull))] = p; // base + rank < IP_PX: at most one entry per pixel of the block
    }
    __syncthreads();
    const int n = (int)s_n;

    // ---- phase 2 + 3: a 16-lane row per outlier, a direction per lane
    const int dir = tid & 15, row = tid >> 4;
    const int dx = (int)((IP_DX_NIB >> (4 * dir)) & 15) - 2, dy = (int)((IP_DY_NIB >> (4 * dir)) & 15) - 2;
    for (int e0 = 0; e0 < n; e0 += IP_T / 16) { // block-uniform trip count: every lane reaches the shuffles below
        const bool active = e0 + row < n;
        const uint32_t p = active ? s_list[e0 + row] : 0;
        const int y = (int)(p / (uint32_t)W), x = (int)(p - (uint32_t)y * (uint32_t)W);
        int hit = -1; // the candidate's pixel index
        bool live = active;
        int qx = x + dx, qy = y + dy;
        while (live) {
            bool in[IP_U];
            u8 o[IP_U];
#pragma unroll
            for (int i = 0; i < IP_U; ++i) { // independent loads, every one bounds-checked
                const int xi = qx + i * dx, yi = qy + i * dy;
                in[i] = (unsigned)xi < (unsigned)W && (unsigned)yi < (unsigned)H;
                o[i] = in[i] ? outl[(uint32_t)yi * (uint32_t)W + (uint32_t)xi] : (u8)1;
            }
#pragma unroll
            for (int i = 0; i < IP_U; ++i) { // ... tested in walk order
                if (live && !in[i]) live = false; // left the image: no candidate
                if (live && o[i] == 0) {
                    hit = (qy + i * dy) * W + (qx + i * dx);
                    live = false;
                }
            }
            qx += IP_U * dx;
            qy += IP_U * dy;
        }
        const bool has = hit >= 0;
        const u8 cls = active ? outl[p] : (u8)0;
        float val = 0.0f;
        int key = 0x7fffffff; // mismatch: colour distance * 16 + direction
        if (has) {
            val = disp[hit];
            if (cls != 2) {
                const u8 *cp = img + (size_t)p * elem_sz, *cq = img + (size_t)hit * elem_sz;
                const int c = abs((int)cq[0] - (int)cp[0]) + abs((int)cq[1] - (int)cp[1]) + abs((int)cq[2] - (int)cp[2]);
                key = c * 16 + dir;
            }
        }
        const uint32_t cand = (uint32_t)(__ballot(has) >> (lane & 48)) & 0xffffu; // the row's directions that have a candidate
        // Both reductions run in every lane (no shuffle under a divergent branch); the row's class picks the winner.
        // Occlusion: v > best never holds with a NaN on either side, so a NaN that comes first stays and a later one never enters.
        const int first = cand ? __ffs((int)cand) - 1 : 0;
        const float vfirst = __shfl(val, first, 16);
        bool ok = has && !(val != val);
        float bv = val;
        int bi = dir;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(bv, m, 16);
            const int oi = __shfl_xor(bi, m, 16);
            const bool ook = __shfl_xor((int)ok, m, 16) != 0;
            if (ook && (!ok || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; ok = true; }
            key = min(key, __shfl_xor(key, m, 16));
        }
        // the direction whose candidate the sequential fold ends with
        const int win = cls == 2 ? ((vfirst != vfirst) ? first : bi) : (key & 15);
        const float res = __shfl(val, win, 16);
        if (active && cand != 0 && dir == 0) disp[p] = res;
    }
}

// disp[v] refined in place on outl[v] (read only) and the view's own image img[v] (elem_sz >= 3 bytes per pixel), v < nviews
void launch_interp(int nviews, float *const *disp, const u8 *const *outl, const u8 *const *img, int H, int W, int elem_sz)
{
    const size_t HW = (size_t)H * W;
    if (nviews < 1 || nviews > 2) {
        fail("launch_interp: 1 or 2 views", "nviews", __FILE__, __LINE__);
        return;
    }
    if (HW >= (1u << 31)) { // pixel indices are 32-bit in the kernel
        fail("dr_interp: more than 2^31 - 1 pixels", "num_rows * num_cols", __FILE__, __LINE__);
        return;
    }
    InterpArgs a;
    for (int v = 0; v < 2; ++v) {
        const int s = v < nviews ? v : 0;
        a.disp[v] = disp[s]; a.outl[v] = outl[s]; a.img[v] = img[s];
    }
    ProfScope p("interp");
    STM_LAUNCH(stm_k_interp, dim3((unsigned)((HW + IP_PX - 1) / IP_PX), nviews), dim3(IP_T), 0, stream(), a, H, W, elem_sz);
    STM_CHECK_LAUNCH();
}

} // namespace stm
