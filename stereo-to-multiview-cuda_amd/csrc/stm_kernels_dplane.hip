// stm_kernels_dplane.hip -- the disparity maps of a frame stream as 8- or 16-bit depth planes (stm_stream_maps, formats 2 and 3):
// the float maps stay on the device, where the temporal history and the renderer read them; what crosses the link is one code per
// pixel, 1 or 2 bytes instead of 4.  An addition: the reference only ever hands out its float maps.
//
// Definition (include/stm_hip.h), f32, one operation per line, per map value d; MAXC = 255 (u8) or 65535 (u16):
//   k = (float)((double)MAXC / ((double)hi - (double)lo))     on the host, once; negative when hi < lo
//   t = d - lo;  t = t * k;                                    (the file is built with -ffp-contract=off: no fma)
//   t = fmaxf(t, 0.0f);  t = fminf(t, (float)MAXC);            (a NaN leaves the fmaxf as 0)
//   code = (unsigned)(t + 0.5f)                                (exact: t + 0.5 <= 65535.5 is an f32)
// u16 codes are stored little-endian, planes are tight (H * W codes, no pitch).
//
// One kernel, stm_k_disp_plane<MAXC>, for one or two maps (blockIdx.y).  It is pure traffic: 4 bytes read and 1 or 2 written per
// pixel, five VALU operations between them.  What decides its shape is the number of memory instructions, not the bytes: stores
// are issue-bound on this chip (a byte or short store costs a whole store instruction, several times a dwordx4 store's time per
// byte, and a store tail of narrow stores queues wave behind wave), and 16 bytes is the widest global access there is.  So a lane
// owns 16 bytes of OUTPUT -- 16 u8 or 8 u16 codes, packed in registers and stored as one dwordx4 -- and reads them as four or two
// float4 loads (dwordx4 as well); a wave's store covers 1 KiB of consecutive bytes and its loads 4 or 2 KiB.  Wider per lane buys
// nothing (no wider instruction exists, and more loads in flight per lane only cost registers in a kernel with no reuse),
// narrower multiplies the store instructions.
//
// Alignment.  The two planes lie tight behind each other in the slot's buffer, so the second one starts at byte H * W * bytes,
// which need not be a multiple of 16.  The vector stores must be: the host hands over `head`, the codes in front of the plane's
// first 16-byte boundary, and the vector body starts behind them.  The float loads of the body then start at element `head`: they
// are 4-byte aligned only, which a global dwordx4 load takes (the type below says so to the compiler); an unaligned load touches
// one more cache line, an unaligned store would be split into partial writes.  The `head` codes in front and the (HW - head) mod 16
// (u8) or mod 8 (u16) behind the body are scalar, one code per thread of block 0: fewer than 32 in all.
#include "stm_common.h"

#include <type_traits>

namespace stm {

constexpr int DP_T = 256; // threads per block

typedef float dp_f4 __attribute__((ext_vector_type(4), aligned(4))); // a float4 load at any float's address

struct DispPlaneArgs { // both maps of a frame share the launch
    const float *src[2];
    u8 *dst[2];
    int head[2]; // codes in front of dst's first 16-byte boundary, at most HW
};

template <int MAXC> __device__ __forceinline__ uint32_t dp_code(float d, float lo, float k)
{
    float t = d - lo;
    t = t * k;
    t = fmaxf(t, 0.0f);
    t = fminf(t, (float)MAXC);
    return (uint32_t)(t + 0.5f);
}

template <int MAXC> __global__ __launch_bounds__(DP_T) void stm_k_disp_plane(DispPlaneArgs a, size_t HW, float lo, float k)
{
    typedef typename std::conditional<MAXC == 255, u8, uint16_t>::type code_t;
    constexpr int CPL = 16 / (int)sizeof(code_t); // codes per lane
    const int v = blockIdx.y;
    const float *__restrict__ src = a.src[v];
    code_t *__restrict__ dst = (code_t *)a.dst[v];
    const size_t head = (size_t)a.head[v];
    const size_t nvec = (HW - head) / CPL, tail0 = head + nvec * CPL;
    const size_t g = (size_t)blockIdx.x * DP_T + threadIdx.x;
    if (g < nvec) {
        const size_t e = head + g * CPL; // e + CPL <= tail0 <= HW
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = 0u;
#pragma unroll
        for (int q = 0; q < CPL / 4; ++q) {
            const dp_f4 f = *(const dp_f4 *)(src + e + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = 4 * q + j; // the lane's c-th code: byte c * sizeof(code_t) of its 16
                w[c * (int)sizeof(code_t) / 4] |= dp_code<MAXC>(f[j], lo, k) << (8 * (c * (int)sizeof(code_t) % 4));
            }
        }
        *(uint4 *)(dst + e) = make_uint4(w[0], w[1], w[2], w[3]); // 16-byte aligned: that is what head is for
    }
    // the codes in front of and behind the vector body: head + (HW - tail0) < 2 * CPL <= DP_T, so block 0 has a thread for each
    if (g < head) dst[g] = (code_t)dp_code<MAXC>(src[g], lo, k);
    if (g < HW - tail0) dst[tail0 + g] = (code_t)dp_code<MAXC>(src[tail0 + g], lo, k);
}

// nviews maps of HW floats each to planes of HW codes: u8 (bytes_per_code 1) or little-endian u16 (2).  dst[v] is 1- or 2-byte
// aligned, src[v] 4-byte aligned.  k as the definition above computes it.
void launch_disp_plane(int nviews, const float *const *src, void *const *dst, size_t HW, int bytes_per_code, float lo, float k)
{
    if (nviews < 1 || nviews > 2 || HW < 1 || (bytes_per_code != 1 && bytes_per_code != 2)) {
        fail("launch_disp_plane: 1 or 2 views, HW >= 1, 1 or 2 bytes per code", "nviews, HW, bytes_per_code", __FILE__, __LINE__);
        return;
    }
    DispPlaneArgs a;
    const size_t cpl = 16 / (size_t)bytes_per_code;
    for (int v = 0; v < 2; ++v) {
        const int s = v < nviews ? v : 0;
        if (!src[s] || !dst[s] || ((uintptr_t)src[s] & 3) || ((uintptr_t)dst[s] & (uintptr_t)(bytes_per_code - 1))) { // the kernel's accesses rest on these
            fail("launch_disp_plane: src must be 4-byte aligned, dst aligned to its codes, neither null", "src, dst", __FILE__, __LINE__);
            return;
        }
        a.src[v] = src[s];
        a.dst[v] = (u8 *)dst[s];
        const size_t head = ((16 - ((uintptr_t)dst[s] & 15)) & 15) / (size_t)bytes_per_code;
        a.head[v] = (int)(head < HW ? head : HW);
    }
    const size_t lanes = HW / cpl + 1; // at least the vector items of either map, and block 0 for the scalar codes
    const dim3 grid((unsigned)((lanes + DP_T - 1) / DP_T), nviews);
    ProfScope p("maps_plane");
    if (bytes_per_code == 1) STM_LAUNCH(stm_k_disp_plane<255>, grid, dim3(DP_T), 0, stream(), a, HW, lo, k);
    else STM_LAUNCH(stm_k_disp_plane<65535>, grid, dim3(DP_T), 0, stream(), a, HW, lo, k);
    STM_CHECK_LAUNCH();
}

} // namespace stm
