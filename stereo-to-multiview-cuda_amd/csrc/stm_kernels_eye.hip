// stm_kernels_eye.hip -- the second eye of an image-plus-depth frame (stm_stream_input_depth; include/stm_depth_input.h has the definition,
// steps A to E, line by line).  An addition: the reference renders from a stereo pair and its own matcher only.
// The given image is the left eye and the given plane its disparity map; the right image and the right map are synthesised here and
// the frame's tail then renders from the two images and the two maps as it does behind the matcher.
//
// One kernel, stm_k_eye<FMT>, one workgroup of 256 threads per image row, everything a row needs in LDS:
//   keys[W]  one 64-bit word per TARGET column.  A source pixel x with disparity d lands on column c = clamp(x + (int)d) and offers
//            (ord(d) << 32) | ~x, where ord is the order-preserving bit pattern of an f32: the LDS 64-bit minimum keeps the smallest
//            d and, among equal d, the largest x (steps B and C).  The minimum commutes, so the result does not depend on the order
//            the lanes arrive in.  A column no source reached keeps the initial all-ones word; its high word 0xffffffff is no
//            ord() of a decoded value (that would be a NaN, and step A hands on none).
//   passes   1. clear;  2. decode + scatter (and disp_l, and the tight copy of the image where the frame has a pitch);
//            3. per lane a contiguous chunk of columns: the last hit column of the chunk and the first one, a block-wide maximum scan
//               upwards and a minimum scan downwards (wave scans by shuffles, the four wave totals through LDS) give every chunk the
//               nearest hit column before and behind it; a second walk leaves L + 1 and R in the low word of every hole's own key
//               (a hole's slot carries nothing else, so the hole runs need no memory of their own);
//            4. the writes: every column reads its key, a hole picks its background side B (step E) and, with fill 1, the mirror
//               column 2 B - k; the colour is gathered from the row of the given image.
// Loads and stores: the plane is read 16 bytes per lane (4 f32, 8 u16 or 16 u8 codes) from the first column of the row whose
// flat index is a multiple of that count -- rows of a tight plane start unaligned when W is odd -- with one code per thread in front
// and behind; both maps leave as float4 on the same grouping, img_r as 12 bytes (3-byte pixels) or 16 bytes (4-byte pixels) per four
// columns.  No global atomics, no scratch in device memory, nothing read back: the launch replays inside a captured graph.
// LDS: 8 W + 64 bytes, 64 KiB + 64 at the largest W the entry takes (8192); above 64 KiB the launch opts in (160 KiB per CU).
//
// A second form, stm_k_eye_video<FMT, AXIS, FILT>, takes a packed 2D-plus-depth video frame (stm_stream_input_packed_depth;
// include/stm_depth_video.h has the definition, steps 0 and A' to A''' line by line): the image is one half of
// a BGR or NV12 frame and the depth a grey picture in the other half.  The same four passes on the same keys; pass 2 takes a pixel of
// the image through stm_fetch.h's gather, expansion and conversion, and the depth sample(s) from the other half, and writes the
// tight img_l; pass 4 gathers the winner's pixel from that row of img_l, as stm_k_eye gathers it from the given image, so no pixel
// is converted twice.  The read is ordered after the store: the row was stored by waves of this same workgroup, the __syncthreads()
// between the passes is a workgroup-scope release / acquire (every wave's stores have left it, vmcnt 0, before any wave passes the
// barrier), and the waves of a workgroup run on one CU, whose vector L1 all their stores and loads go through in order -- a line of
// it that another workgroup of the CU had fetched for the end of the neighbouring row is updated by the store, not left stale.  No
// other workgroup writes these bytes.  LDS: 8 W + 64 bytes, as stm_k_eye.
// stm_k_eye<FMT> is not touched by it: pass 3 is repeated in the new form, as the fronts repeat each other's phases.
#include "stm_common.h"
#include "stm_fetch.h"

#include <type_traits>

namespace stm {

namespace {

constexpr int EYE_T = 256;                 // threads per block
constexpr uint32_t EYE_HOLE = 0xffffffffu; // the high word of a column no source reached

typedef float eye_f4 __attribute__((ext_vector_type(4)));

struct EyeArgs {
    const u8 *img;       // the given image: H rows of pitch_px pixels of E bytes
    const void *plane;   // H x W codes, tight, 16-byte aligned
    u8 *img_l;           // the tight copy of the image, or null (pitch_px == W: the given image is tight)
    u8 *img_r;           // H x W x E
    float *disp_l, *disp_r;
    int W, pitch_px, E, fill;
    float lo, q, dmin, dmax, gate;
};

__device__ __forceinline__ uint32_t eye_ord(float d)
{
    const uint32_t b = __float_as_uint(d + 0.0f); // -0 and +0 are equal: both compete as +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float eye_unord(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// step A
template <int FMT> __device__ __forceinline__ float eye_decode(const EyeArgs &a, float v)
{
    if (FMT == 0) {
        const float t = fminf(v, a.dmax); // a NaN becomes dmax
        return fmaxf(t, a.dmin);
    }
    const float t = v * a.q; // v = (float)code
    return a.lo + t;
}

// steps B and C for source column x
__device__ __forceinline__ void eye_offer(unsigned long long *keys, int W, int x, float d)
{
    int c = x + (int)d;
    c = c < 0 ? 0 : c > W - 1 ? W - 1 : c;
    atomicMin(&keys[c], ((unsigned long long)eye_ord(d) << 32) | (unsigned long long)(uint32_t)~(uint32_t)x);
}

// the three colour bytes of source pixel x of the row
__device__ __forceinline__ uint32_t eye_px(const u8 *__restrict__ row, int x, int E, int W)
{
    x = (unsigned)x < (unsigned)W ? x : 0; // a key always holds a column of the row; no read leaves it whatever a key holds
    const u8 *p = row + (size_t)x * E;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}
// a whole pixel: the three bytes, zeros behind them
__device__ __forceinline__ void eye_put(u8 *__restrict__ dst, uint32_t bgr, int E)
{
    if (E == 4) {
        *(uint32_t *)dst = bgr; // (flat pixel index) * 4 from a 4-byte aligned base
        return;
    }
    dst[0] = (u8)bgr;
    dst[1] = (u8)(bgr >> 8);
    dst[2] = (u8)(bgr >> 16);
    for (int j = 3; j < E; ++j) dst[j] = 0;
}

// steps D and E for target column k: the source column of its colour and its map value
__device__ __forceinline__ void eye_resolve(const uint2 *__restrict__ kw, const EyeArgs &a, int k, int &src, float &d)
{
    const int W = a.W;
    const uint2 s = kw[k]; // x = low word, y = high word
    if (s.y != EYE_HOLE) {
        src = (int)~s.x;
        d = eye_unord(s.y);
        return;
    }
    const int L = (int)(s.x & 0xffffu) - 1, R = (int)(s.x >> 16); // L = -1, R = W: that side does not exist
    int B;
    if (L >= 0 && R < W) B = eye_unord(kw[L].y) > eye_unord(kw[R].y) ? L : R; // the farther side; a tie goes to R
    else B = L >= 0 ? L : R;
    const uint2 sb = kw[B];
    d = eye_unord(sb.y);
    src = (int)~sb.x;
    if (a.fill == 1) {
        const int m = 2 * B - k;
        if (m >= 0 && m < W) {
            const uint2 sm = kw[m];
            if (sm.y != EYE_HOLE) {
                const float diff = eye_unord(sm.y) - d;
                if (fabsf(diff) <= a.gate) src = (int)~sm.x;
            }
        }
    }
}

template <int FMT> __global__ __launch_bounds__(EYE_T) void stm_k_eye(EyeArgs a)
{
    typedef typename std::conditional<FMT == 0, float, typename std::conditional<FMT == 2, u8, uint16_t>::type>::type code_t;
    constexpr int CPL = 16 / (int)sizeof(code_t); // codes per lane and load
    extern __shared__ unsigned long long eye_lds[];
    const int W = a.W, E = a.E, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long *keys = eye_lds;
    int *tot = (int *)(eye_lds + W); // [0 .. 3]: the waves' last hit columns, [4 .. 7]: their first ones
    const size_t y = blockIdx.x, flat0 = y * (size_t)W;
    const u8 *__restrict__ row = a.img + y * (size_t)a.pitch_px * E;
    const code_t *__restrict__ codes = (const code_t *)a.plane + flat0;
    float *__restrict__ dl = a.disp_l + flat0;
    float *__restrict__ dr = a.disp_r + flat0;

    for (int k = tid; k < W; k += EYE_T) keys[k] = ~0ull;
    __syncthreads();

    // ---- pass 2: decode, scatter, disp_l.  Columns [0, head) and [tail0, W) one per thread, the groups of CPL between them by lanes
    {
        const int mis = (int)(flat0 % CPL);
        int head = mis ? CPL - mis : 0;
        head = head < W ? head : W;
        const int nvec = (W - head) / CPL, tail0 = head + nvec * CPL;
        for (int g = tid; g < nvec; g += EYE_T) {
            const int k0 = head + g * CPL; // flat0 + k0 is a multiple of CPL: the 16 bytes are aligned
            const uint4 raw = *(const uint4 *)(codes + k0);
            const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
            for (int q4 = 0; q4 < CPL / 4; ++q4) {
                eye_f4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = 4 * q4 + j;
                    float v;
                    if (FMT == 0) v = __uint_as_float(w[c]);
                    else if (FMT == 2) v = (float)((w[c >> 2] >> (8 * (c & 3))) & 0xffu);
                    else v = (float)((w[c >> 1] >> (16 * (c & 1))) & 0xffffu);
                    const float d = eye_decode<FMT>(a, v);
                    eye_offer(keys, W, k0 + c, d);
                    o[j] = d;
                }
                *(eye_f4 *)(dl + k0 + 4 * q4) = o;
            }
        }
        if (tid < head) {
            const float d = eye_decode<FMT>(a, (float)codes[tid]);
            eye_offer(keys, W, tid, d);
            dl[tid] = d;
        }
        if (tid < W - tail0) { // fewer than CPL <= 16 columns
            const int k = tail0 + tid;
            const float d = eye_decode<FMT>(a, (float)codes[k]);
            eye_offer(keys, W, k, d);
            dl[k] = d;
        }
        if (a.img_l) { // the frame has a pitch: the left image the tail reads is a tight copy
            u8 *__restrict__ out = a.img_l + flat0 * E;
            for (int k = tid; k < W; k += EYE_T) eye_put(out + (size_t)k * E, eye_px(row, k, E, W), E);
        }
    }
    __syncthreads();

    // ---- pass 3: the nearest hit column before and behind every hole
    {
        uint2 *kw = (uint2 *)keys;
        const int CH = (W + EYE_T - 1) / EYE_T;
        const int s = tid * CH < W ? tid * CH : W, e = s + CH < W ? s + CH : W;
        int last = -1, first = W;
        for (int k = s; k < e; ++k)
            if (kw[k].y != EYE_HOLE) {
                last = k;
                first = first == W ? k : first;
            }
        int up = last, down = first; // inclusive scans inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(up, o), v = __shfl_down(down, o);
            if (lane >= o) up = up > u ? up : u;
            if (lane + o < 64) down = down < v ? down : v;
        }
        int L = __shfl_up(up, 1), R = __shfl_down(down, 1); // exclusive
        if (lane == 0) L = -1;
        if (lane == 63) R = W;
        if (lane == 63) tot[wave] = up;
        if (lane == 0) tot[4 + wave] = down;
        __syncthreads();
        for (int i = 0; i < 4; ++i) {
            if (i < wave) L = L > tot[i] ? L : tot[i];
            if (i > wave) R = R < tot[4 + i] ? R : tot[4 + i];
        }
        for (int k = s; k < e; ++k) {
            if (kw[k].y != EYE_HOLE) L = k;
            else kw[k].x = (uint32_t)(L + 1);
        }
        for (int k = e - 1; k >= s; --k) {
            if (kw[k].y != EYE_HOLE) R = k;
            else kw[k].x |= (uint32_t)R << 16;
        }
    }
    __syncthreads();

    // ---- pass 4: the writes, four columns per lane on the float4 grouping of the row
    {
        const uint2 *kw = (const uint2 *)keys;
        u8 *__restrict__ out = a.img_r + flat0 * E;
        const int mis = (int)(flat0 & 3);
        int head = mis ? 4 - mis : 0;
        head = head < W ? head : W;
        const int nvec = (W - head) / 4, tail0 = head + nvec * 4;
        for (int g = tid; g < nvec; g += EYE_T) {
            const int k0 = head + g * 4;
            eye_f4 o;
            uint32_t px[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int src;
                float d;
                eye_resolve(kw, a, k0 + j, src, d);
                o[j] = d;
                px[j] = eye_px(row, src, E, W);
            }
            *(eye_f4 *)(dr + k0) = o;
            u8 *p = out + (size_t)k0 * E;
            if (E == 3) { // 12 bytes at a multiple of 12 from a 4-byte aligned base
                uint32_t *p32 = (uint32_t *)p;
                p32[0] = px[0] | (px[1] << 24);
                p32[1] = (px[1] >> 8) | (px[2] << 16);
                p32[2] = (px[2] >> 16) | (px[3] << 8);
            } else if (E == 4) {
                *(uint4 *)p = make_uint4(px[0], px[1], px[2], px[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) eye_put(p + (size_t)j * E, px[j], E);
            }
        }
        const int k = tid < head ? tid : tail0 + (tid - head); // head + (W - tail0) < 8 columns, one per thread
        if (tid < head + (W - tail0)) {
            int src;
            float d;
            eye_resolve(kw, a, k, src, d);
            dr[k] = d;
            eye_put(out + (size_t)k * E, eye_px(row, src, E, W), E);
        }
    }
}

// ---------------------------------------------------------------- packed 2D-plus-depth video frames
struct EyeVideoArgs {
    EyeArgs e;  // img_l (never null here), img_r, disp_l, disp_r, W, E, fill, gate, lo and q (= q4); the other members are not read
    AlignSrc s; // the packed frame: eye 0 is the image, eye 1 the depth picture
    int dfilter, dgate, cmin, cmax; // step A': c = min(max(sample, cmin), cmax) - cmin; range 0: 0 and 255, range 1: 16 and 235
};

// step A': the code of sample i (along the packing axis) of the depth picture at the other coordinate o.  NV12: the Y byte; BGR: G
template <int FMT, int AXIS> __device__ __forceinline__ int video_code(const EyeVideoArgs &a, int i, int o)
{
    const int row = AXIS == 0 ? o : a.s.org[1] + i, col = AXIS == 0 ? a.s.org[1] + i : o;
    const size_t px = (size_t)row * a.s.pitch0 + col;
    const int smp = FMT == 0 ? a.s.p0[1][px * a.s.elem_sz + 1] : a.s.p0[1][px];
    return min(max(smp, a.cmin), a.cmax) - a.cmin;
}
// steps A'' and A''' for pixel (x, y) of the image
template <int FMT, int AXIS, int FILT> __device__ __forceinline__ float video_depth(const EyeVideoArgs &a, int y, int x)
{
    const int ax = AXIS == 0 ? x : y, o = AXIS == 0 ? y : x;
    int v;
    if (FILT == 0) {
        v = 4 * video_code<FMT, AXIS>(a, ax, o);
    } else {
        const int k = ax >> 1, c0 = video_code<FMT, AXIS>(a, k, o);
        v = 4 * c0;
        if (a.dfilter) { // the neighbour clamps inside the depth picture's own region
            const int sg = (ax & 1) ? 1 : -1, c1 = video_code<FMT, AXIS>(a, min(max(k + sg, 0), a.s.n - 1), o);
            if (abs(c0 - c1) <= a.dgate) v = 3 * c0 + c1;
        }
    }
    const float t = (float)v * a.e.q;
    return a.e.lo + t;
}
// four pixels from a column whose flat index is a multiple of 4: 12 bytes (3-byte pixels) or 16 (4-byte pixels), as stm_k_eye's pass 4
__device__ __forceinline__ void eye_put4(u8 *__restrict__ p, const uint32_t px[4], int E)
{
    if (E == 3) {
        uint32_t *p32 = (uint32_t *)p;
        p32[0] = px[0] | (px[1] << 24);
        p32[1] = (px[1] >> 8) | (px[2] << 16);
        p32[2] = (px[2] >> 16) | (px[3] << 8);
    } else if (E == 4) {
        *(uint4 *)p = make_uint4(px[0], px[1], px[2], px[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) eye_put(p + (size_t)j * E, px[j], E);
    }
}

// FMT 0 = BGR, 1 = NV12; AXIS 0 = the halves lie side by side, 1 = one above the other; FILT 0 = copy, 1 = linear, 2 = Catmull-Rom
template <int FMT, int AXIS, int FILT> __global__ __launch_bounds__(EYE_T) void stm_k_eye_video(EyeVideoArgs a)
{
    extern __shared__ unsigned long long eye_lds[];
    const int W = a.e.W, E = a.e.E, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, y = (int)blockIdx.x;
    unsigned long long *keys = eye_lds;
    int *tot = (int *)(eye_lds + W); // as stm_k_eye's
    const size_t flat0 = (size_t)y * W;
    float *__restrict__ dl = a.e.disp_l + flat0;
    float *__restrict__ dr = a.e.disp_r + flat0;
    const int mis = (int)(flat0 & 3); // both passes that write: four columns per lane on the float4 grouping of the row
    int head = mis ? 4 - mis : 0;
    head = head < W ? head : W;
    const int nvec = (W - head) / 4, tail0 = head + nvec * 4;
    const int kedge = tid < head ? tid : tail0 + (tid - head); // head + (W - tail0) < 8 columns, one per thread
    const bool edge = tid < head + (W - tail0);

    for (int k = tid; k < W; k += EYE_T) keys[k] = ~0ull;
    __syncthreads();

    // ---- pass 2: steps 0 and A' to A''', the offer, disp_l and img_l
    {
        u8 *out = a.e.img_l + flat0 * E; // (no __restrict__: pass 4 reads this row back)
        auto column = [&](int x, float &d) {
            const uint32_t px = al_unpacked_px<FMT, AXIS, FILT>(a.s, 0, y, x);
            d = video_depth<FMT, AXIS, FILT>(a, y, x);
            eye_offer(keys, W, x, d);
            return px;
        };
        for (int g = tid; g < nvec; g += EYE_T) {
            const int k0 = head + g * 4;
            eye_f4 o;
            uint32_t px[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float d;
                px[j] = column(k0 + j, d);
                o[j] = d;
            }
            *(eye_f4 *)(dl + k0) = o;
            eye_put4(out + (size_t)k0 * E, px, E);
        }
        if (edge) {
            float d;
            const uint32_t px = column(kedge, d);
            dl[kedge] = d;
            eye_put(out + (size_t)kedge * E, px, E);
        }
    }
    __syncthreads();

    // ---- pass 3: stm_k_eye's, line by line
    {
        uint2 *kw = (uint2 *)keys;
        const int CH = (W + EYE_T - 1) / EYE_T;
        const int s = tid * CH < W ? tid * CH : W, e = s + CH < W ? s + CH : W;
        int last = -1, first = W;
        for (int k = s; k < e; ++k)
            if (kw[k].y != EYE_HOLE) {
                last = k;
                first = first == W ? k : first;
            }
        int up = last, down = first;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(up, o), v = __shfl_down(down, o);
            if (lane >= o) up = up > u ? up : u;
            if (lane + o < 64) down = down < v ? down : v;
        }
        int L = __shfl_up(up, 1), R = __shfl_down(down, 1);
        if (lane == 0) L = -1;
        if (lane == 63) R = W;
        if (lane == 63) tot[wave] = up;
        if (lane == 0) tot[4 + wave] = down;
        __syncthreads();
        for (int i = 0; i < 4; ++i) {
            if (i < wave) L = L > tot[i] ? L : tot[i];
            if (i > wave) R = R < tot[4 + i] ? R : tot[4 + i];
        }
        for (int k = s; k < e; ++k) {
            if (kw[k].y != EYE_HOLE) L = k;
            else kw[k].x = (uint32_t)(L + 1);
        }
        for (int k = e - 1; k >= s; --k) {
            if (kw[k].y != EYE_HOLE) R = k;
            else kw[k].x |= (uint32_t)R << 16;
        }
    }
    __syncthreads();

    // ---- pass 4: the writes; the colour is gathered from the row of img_l this workgroup stored in pass 2 (the file's head)
    {
        const uint2 *kw = (const uint2 *)keys;
        u8 *__restrict__ out = a.e.img_r + flat0 * E;
        const u8 *lrow = a.e.img_l + flat0 * E;
        auto column = [&](int k, float &d) {
            int src;
            eye_resolve(kw, a.e, k, src, d);
            return eye_px(lrow, src, E, W);
        };
        for (int g = tid; g < nvec; g += EYE_T) {
            const int k0 = head + g * 4;
            eye_f4 o;
            uint32_t px[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float d;
                px[j] = column(k0 + j, d);
                o[j] = d;
            }
            *(eye_f4 *)(dr + k0) = o;
            eye_put4(out + (size_t)k0 * E, px, E);
        }
        if (edge) {
            float d;
            const uint32_t px = column(kedge, d);
            dr[kedge] = d;
            eye_put(out + (size_t)kedge * E, px, E);
        }
    }
}

struct EyeVideoLaunch {
    EyeVideoArgs a;
    int H;
    template <int FMT, int AXIS, int FILT> void run() const
    {
        const size_t lds = (size_t)a.e.W * 8 + 64;
        if (lds > 64 * 1024) // no stream operation
            STM_CHECK(hipFuncSetAttribute((const void *)stm_k_eye_video<FMT, AXIS, FILT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        STM_LAUNCH((stm_k_eye_video<FMT, AXIS, FILT>), dim3((unsigned)H), dim3(EYE_T), lds, stream(), a);
    }
};

} // namespace

// The second eye of an image-plus-depth frame (the file's head; steps A to E of stm_stream_input_depth).  img: H rows of pitch_px
// pixels of elem_sz bytes, of which the first W are read; plane: H x W codes of `format` (0 = f32, 2 = u8, 3 = u16), tight and
// 16-byte aligned; img_l: the tight copy of the image, or null where pitch_px == W; img_r, disp_l, disp_r: tight, 16-byte aligned.
// 1 <= W <= 8192.  Screened by the caller; what the kernel's accesses rest on is checked here again.
void launch_depth_eye(const u8 *img, int pitch_px, const void *plane, int format, float lo, float hi, int fill, float gate, u8 *img_l,
                      u8 *img_r, float *disp_l, float *disp_r, int H, int W, int elem_sz)
{
    if (H < 1 || W < 1 || W > 8192 || pitch_px < W || elem_sz < 3 || (format != 0 && format != 2 && format != 3) || (fill != 0 && fill != 1)) {
        fail("launch_depth_eye: H >= 1, 1 <= W <= 8192, pitch >= W, elem_sz >= 3, format 0, 2 or 3, fill 0 or 1",
             "H, W, pitch_px, elem_sz, format, fill", __FILE__, __LINE__);
        return;
    }
    if (!img || !plane || !img_r || !disp_l || !disp_r || (!img_l && pitch_px != W) || ((uintptr_t)plane & 15) || ((uintptr_t)disp_l & 15) ||
        ((uintptr_t)disp_r & 15) || ((uintptr_t)img_r & 15) || ((uintptr_t)img_l & 3)) {
        fail("launch_depth_eye: no null pointer, plane, img_r, disp_l and disp_r 16-byte aligned, img_l 4-byte aligned", "pointers", __FILE__,
             __LINE__);
        return;
    }
    EyeArgs a;
    a.img = img; a.plane = plane; a.img_l = img_l; a.img_r = img_r; a.disp_l = disp_l; a.disp_r = disp_r;
    a.W = W; a.pitch_px = pitch_px; a.E = elem_sz; a.fill = fill;
    const int maxcode = format == 2 ? 255 : 65535;
    a.lo = lo;
    a.q = format == 0 ? 0.0f : (float)(((double)hi - (double)lo) / (double)maxcode);
    a.dmin = fminf(lo, hi);
    a.dmax = fmaxf(lo, hi);
    a.gate = gate;
    const size_t lds = (size_t)W * 8 + 64;
    const void *fn = format == 0 ? (const void *)stm_k_eye<0> : format == 2 ? (const void *)stm_k_eye<2> : (const void *)stm_k_eye<3>;
    if (lds > 64 * 1024) STM_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); // no stream operation
    ProfScope p("depth_eye");
    if (format == 0) STM_LAUNCH(stm_k_eye<0>, dim3((unsigned)H), dim3(EYE_T), lds, stream(), a);
    else if (format == 2) STM_LAUNCH(stm_k_eye<2>, dim3((unsigned)H), dim3(EYE_T), lds, stream(), a);
    else STM_LAUNCH(stm_k_eye<3>, dim3((unsigned)H), dim3(EYE_T), lds, stream(), a);
    STM_CHECK_LAUNCH();
}

// The second eye of a packed 2D-plus-depth video frame (the file's head; stm_stream_input_packed_depth).  in: the frame as the cut and
// active preludes take it, BGR or NV12 under dv.pk; eye 0 of the packing is the image, eye 1 the depth picture.  img_l, img_r, disp_l,
// disp_r: tight, 16-byte aligned.  1 <= W <= 8192.  Screened by the caller; what the kernel's accesses rest on is checked here again.
void launch_depth_eye_video(const PackInput &in, const DepthVideo &dv, u8 *img_l, u8 *img_r, float *disp_l, float *disp_r, int H, int W,
                            int elem_sz)
{
    if (H < 1 || W < 1 || W > 8192 || elem_sz < 3 || (dv.fill != 0 && dv.fill != 1) || (dv.range != 0 && dv.range != 1) ||
        (dv.dfilter != 0 && dv.dfilter != 1) || (dv.dfilter && !(dv.pk.packing & 1)) || dv.dgate < 0 || dv.dgate > 255) {
        fail("launch_depth_eye_video: H >= 1, 1 <= W <= 8192, elem_sz >= 3, fill, range and dfilter 0 or 1, dfilter 1 with packing 1 or 3 only, "
             "dgate 0 .. 255", "H, W, elem_sz, fill, range, dfilter, dgate", __FILE__, __LINE__);
        return;
    }
    // every read of the two halves stays inside the frame this rule describes
    if (!packing_args_ok("launch_depth_eye_video", in.pk, H, in.nv12 ? in.pitch_y : in.num_cols_sbs, W, "num_cols", in.nv12, in.pitch_y,
                         in.pitch_uv, in.matrix))
        return;
    if (!(in.nv12 ? in.y && in.uv : in.frame != nullptr) || !img_l || !img_r || !disp_l || !disp_r || ((uintptr_t)disp_l & 15) ||
        ((uintptr_t)disp_r & 15) || ((uintptr_t)img_l & 15) || ((uintptr_t)img_r & 15)) {
        fail("launch_depth_eye_video: no null pointer, img_l, img_r, disp_l and disp_r 16-byte aligned", "pointers", __FILE__, __LINE__);
        return;
    }
    EyeVideoLaunch l;
    l.H = H;
    EyeArgs &e = l.a.e;
    e.img = nullptr; e.plane = nullptr; e.img_l = img_l; e.img_r = img_r; e.disp_l = disp_l; e.disp_r = disp_r;
    e.W = W; e.pitch_px = W; e.E = elem_sz; e.fill = dv.fill;
    e.lo = dv.lo;
    e.q = (float)(((double)dv.hi - (double)dv.lo) / (4.0 * (dv.range ? 219 : 255))); // q4 of step A'''
    e.dmin = e.dmax = 0.0f;
    e.gate = dv.gate;
    l.a.s = make_src(&in, nullptr, nullptr, H, W, elem_sz);
    l.a.dfilter = dv.dfilter; l.a.dgate = dv.dgate;
    l.a.cmin = dv.range ? 16 : 0; l.a.cmax = dv.range ? 235 : 255;
    ProfScope p("depth_eye_video");
    dispatch(&in, l);
    STM_CHECK_LAUNCH();
}

} // namespace stm
