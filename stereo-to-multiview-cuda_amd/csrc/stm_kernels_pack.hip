// stm_kernels_pack.hip -- packed stereo frames (stm_set_packing, include/stm_hip.h): half-width side-by-side, top-and-bottom (full,
// half, with a gap), either eye first, as BGR or NV12.  An addition: the reference takes two full-resolution eyes side by side only.
// Two kernels, both templates over the input format, the packing axis and the filter, so that a fetch carries no branch on them:
//   stm_k_demux_packed   the stage (stm_d_demux_packed / stm_d_demux_nv12_packed): one thread per pixel of the two unpacked eyes;
//   stm_k_front_pack     the frame's first kernel under a packing: stm_k_front's tile and phases (stm_kernels_cost.hip) with a fetch
//                        that gathers, filters and, for NV12, converts.  No unpacked side-by-side frame is materialised.
// stm_k_front and stm_k_front_nv12 are not touched and share no text with this file: the default path must not move (DESIGN.md
// sections 14 and 17), so the store and census phases are repeated here by hand, as in stm_k_front_nv12.
#include "stm_common.h"

namespace stm {

namespace {

// the conversion of stm_demux_nv12 (stm_hip.h): the table and the arithmetic of stm_kernels_cost.hip, repeated because that file
// keeps them private
struct PkNv12Coef { int ky, rv, gu, gv, bu, yo; };
const PkNv12Coef PK_NV12_COEF[4] = {
    {76309, 104597, 25675, 53279, 132201, 16}, // 0: BT.601 limited range
    {76309, 117489, 13975, 34925, 138438, 16}, // 1: BT.709 limited range
    {65536, 91881, 22553, 46802, 116130, 0},   // 2: BT.601 full range
    {65536, 103206, 12276, 30679, 121609, 0},  // 3: BT.709 full range
};
__device__ __forceinline__ uint32_t pk_nv12_bgrx(int Y, int U, int V, const PkNv12Coef &c)
{
    const int C = Y - c.yo, D = U - 128, E = V - 128, k = c.ky * C + 32768;
    const int b = min(max((k + c.bu * D) >> 16, 0), 255);
    const int g = min(max((k - c.gu * D - c.gv * E) >> 16, 0), 255);
    const int r = min(max((k + c.rv * E) >> 16, 0), 255);
    return (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16);
}
// grey = (u8)(b*c + g*c + r*c) as stm_kernels_cost.hip's grey_of (d_mux_common.cu:16-20)
__device__ __forceinline__ uint32_t pk_grey_of(uint32_t px)
{
    const float c = 0.33333334f;
    float b = (float)(px & 0xff) * c;
    float g = (float)((px >> 8) & 0xff) * c;
    float r = (float)((px >> 16) & 0xff) * c;
    float s = b + g;
    s = s + r;
    return (uint32_t)s;
}

// Where the two eyes lie.  p0: the BGR frame or the Y plane, p1: the UV plane; pitch0 in pixels (BGR) or bytes (Y), pitch1 in bytes.
// org[e]: the first column (AXIS 0) or row (AXIS 1) of eye e in the frame, n: the packed eye's samples along the packing axis.
struct PackSrc {
    const u8 *p0, *p1;
    int pitch0, pitch1, elem_sz;
    int org[2], n;
    PkNv12Coef c;
};

// FMT 0 = BGR, 1 = NV12; the frame's pixel (row, col) as a BGRX dword
template <int FMT> __device__ __forceinline__ uint32_t frame_px(const PackSrc &s, int row, int col)
{
    if (FMT == 0) {
        const u8 *p = s.p0 + ((size_t)row * s.pitch0 + col) * s.elem_sz;
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
    const int Y = s.p0[(size_t)row * s.pitch0 + col];
    const u8 *q = s.p1 + (size_t)(row >> 1) * s.pitch1 + (col & ~1); // chroma replicated at packed resolution, in frame coordinates
    return pk_nv12_bgrx(Y, q[0], q[1], s.c);
}
// AXIS 0 = the eyes lie side by side (the packing axis is x), 1 = one above the other (y); sample i of eye e along that axis, at
// the other coordinate o
template <int FMT, int AXIS> __device__ __forceinline__ uint32_t eye_px(const PackSrc &s, int e, int i, int o)
{
    return AXIS == 0 ? frame_px<FMT>(s, o, s.org[e] + i) : frame_px<FMT>(s, s.org[e] + i, o);
}
// one byte of the expansion by two (stm_hip.h): (w0 a + w1 b + w2 c + w3 d + 64) >> 7, clipped
__device__ __forceinline__ int pk_clip255(int v) { return min(max(v, 0), 255); }
// FILT 0 = copy (the full packings), 1 = linear, 2 = Catmull-Rom.  Pixel (x, y) of unpacked eye e, 0 <= x < W, 0 <= y < H.
template <int FMT, int AXIS, int FILT> __device__ __forceinline__ uint32_t unpacked_px(const PackSrc &s, int e, int y, int x)
{
    const int a = AXIS == 0 ? x : y, o = AXIS == 0 ? y : x;
    if (FILT == 0) return eye_px<FMT, AXIS>(s, e, a, o);
    const int k = a >> 1, sg = (a & 1) ? 1 : -1, last = s.n - 1;
    // indices clamp to the eye's own region: never into the gap or the other eye
    const uint32_t p1 = eye_px<FMT, AXIS>(s, e, k, o), p2 = eye_px<FMT, AXIS>(s, e, min(max(k + sg, 0), last), o);
    uint32_t out = 0;
    if (FILT == 1) {
#pragma unroll
        for (int c = 0; c < 24; c += 8) {
            const int v = (96 * (int)((p1 >> c) & 0xff) + 32 * (int)((p2 >> c) & 0xff) + 64) >> 7;
            out |= (uint32_t)pk_clip255(v) << c;
        }
        return out;
    }
    const uint32_t p0 = eye_px<FMT, AXIS>(s, e, min(max(k - sg, 0), last), o), p3 = eye_px<FMT, AXIS>(s, e, min(max(k + 2 * sg, 0), last), o);
#pragma unroll
    for (int c = 0; c < 24; c += 8) {
        const int v = (-9 * (int)((p0 >> c) & 0xff) + 111 * (int)((p1 >> c) & 0xff) + 29 * (int)((p2 >> c) & 0xff) -
                       3 * (int)((p3 >> c) & 0xff) + 64) >> 7;
        out |= (uint32_t)pk_clip255(v) << c;
    }
    return out;
}

// ---------------------------------------------------------------- the stage: one thread per pixel of the two unpacked eyes
template <int FMT, int AXIS, int FILT>
__global__ __launch_bounds__(256) void stm_k_demux_packed(u8 *__restrict__ l, u8 *__restrict__ r, PackSrc s, int W)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= 2 * W) return;
    const bool right = x >= W;
    const int ex = right ? x - W : x;
    const uint32_t px = unpacked_px<FMT, AXIS, FILT>(s, right ? 1 : 0, y, ex);
    u8 *d = (right ? r : l) + ((size_t)y * W + ex) * s.elem_sz;
    d[0] = (u8)px; d[1] = (u8)(px >> 8); d[2] = (u8)(px >> 16);
}

// ---------------------------------------------------------------- the frame's first kernel under a packing
// stm_k_front (stm_kernels_cost.hip) phase by phase and line by line -- see there for the tile, the halo trips, the dword stores of
// the split image and the census phase -- with the fetch above: the halo clamps to the edge of the UNPACKED eye, which is what
// stm_k_front does on the unpacked side-by-side frame, so every plane it writes is that kernel's on that frame, bit for bit.
constexpr int PF_TX = 64, PF_TY = 16;
template <int FMT, int AXIS, int FILT>
__global__ __launch_bounds__(256) void stm_k_front_pack(u8 *__restrict__ l, u8 *__restrict__ r, uint32_t *__restrict__ pk_l,
                                                        uint32_t *__restrict__ pk_r, uint32_t *__restrict__ wide_l,
                                                        uint32_t *__restrict__ wide_r, uint32_t *__restrict__ cen_l,
                                                        uint32_t *__restrict__ cen_r, PackSrc s, int H, int W)
{
    constexpr int TW = PF_TX + 8, TH = PF_TY + 4;
    __shared__ __attribute__((aligned(16))) u8 g[TH][TW + 4]; // (a row is 76 bytes: dword reads of a row stay aligned)
    const int view = blockIdx.z, x0 = blockIdx.x * PF_TX, y0 = blockIdx.y * PF_TY, tid = threadIdx.x, elem_sz = s.elem_sz;
    u8 *__restrict__ img = view ? r : l;
    uint32_t *__restrict__ pk = view ? pk_r : pk_l, *__restrict__ wide = view ? wide_r : wide_l, *__restrict__ census = view ? cen_r : cen_l;
    const int lane = tid & 63, wave = tid >> 6;
    auto fetch = [&](int ty, int tx) {
        const int gx = min(max(x0 + tx - 4, 0), W - 1), gy = min(max(y0 + ty - 1, 0), H - 1); // clamp-to-edge inside the unpacked eye
        return unpacked_px<FMT, AXIS, FILT>(s, view, gy, gx);
    };
    constexpr int NH = TW * TH - PF_TX * PF_TY; // halo elements
    uint32_t own[PF_TY / 4], halo[2];
    int hty[2], htx[2];
#pragma unroll
    for (int k = 0; k < PF_TY / 4; ++k) own[k] = fetch(wave + 4 * k + 1, lane + 4);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int h = min(tid + 256 * m, NH - 1);
        if (h < 4 * TW) {
            const int q = h / TW;
            hty[m] = q == 0 ? 0 : PF_TY + q;
            htx[m] = h - q * TW;
        } else {
            const int e = h - 4 * TW;
            hty[m] = 1 + (e >> 3);
            htx[m] = (e & 7) < 4 ? (e & 7) : PF_TX + (e & 7);
        }
        halo[m] = fetch(hty[m], htx[m]);
    }
    // the split image as dwords: 64 pixels of 3 bytes are 48 aligned dwords of the row, each built from two neighbouring pixels
    const bool img_dwords = elem_sz == 3 && (W & 3) == 0 && x0 + PF_TX <= W && (((uintptr_t)img) & 3) == 0;
    const int p0 = (4 * lane) / 3, o8 = 8 * (4 * lane - 3 * p0); // lane < 48: dword `lane` starts in byte o8 / 8 of pixel p0
#pragma unroll
    for (int k = 0; k < PF_TY / 4; ++k) {
        const int rw = wave + 4 * k, ux = x0 + lane, uy = y0 + rw;
        g[rw + 1][lane + 4] = (u8)pk_grey_of(own[k]);
        if (uy >= H) continue; // (the whole wave)
        const uint32_t b = own[k] & 0xff, gg = (own[k] >> 8) & 0xff, rr = own[k] >> 16;
        const size_t p = (size_t)uy * W + ux;
        if (img_dwords) {
            const uint32_t lo = (uint32_t)__shfl((int)own[k], p0 & 63), hi = (uint32_t)__shfl((int)own[k], (p0 + 1) & 63);
            if (lane < 48) ((uint32_t *)(img + ((size_t)uy * W + x0) * 3))[lane] = (uint32_t)((lo | ((unsigned long long)hi << 24)) >> o8);
        } else if (ux < W) {
            u8 *d = img + p * elem_sz;
            d[0] = (u8)b; d[1] = (u8)gg; d[2] = (u8)rr;
        }
        if (ux < W) {
            pk[p] = own[k];
            wide[p] = b | (gg << 10) | (rr << 20);
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
        if (tid + 256 * m < NH) g[hty[m]][htx[m]] = (u8)pk_grey_of(halo[m]);
    __syncthreads();
    const int col = tid & 63, band = tid >> 6, gx = x0 + col; // rows y0 + 4 band .. + 3 of column gx
    if (gx >= W) return;
    uint32_t lo[8], ct[8], hi[8];
    const int a8 = (col & 3) * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t *rw = (const uint32_t *)&g[band * 4 + k][col & ~3];
        const uint32_t d0 = rw[0], d1 = rw[1], d2 = rw[2];
        const unsigned long long q01 = d0 | ((unsigned long long)d1 << 32), q12 = d1 | ((unsigned long long)d2 << 32);
        lo[k] = (uint32_t)(q01 >> a8);
        ct[k] = (uint32_t)(q12 >> a8) & 0xffu;
        hi[k] = (uint32_t)(q12 >> (a8 + 8));
    }
    // bit order of stm_k_census32: window rows -1, +1, +2, +3, in a row x = -4 .. 4 without 0, appended MSB first
    auto row_bits = [](uint32_t lo4, uint32_t hi4, uint32_t cmp) {
        uint32_t b = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) b = (b << 1) | (((lo4 >> (8 * k)) & 0xffu) < cmp ? 1u : 0u);
#pragma unroll
        for (int k = 0; k < 4; ++k) b = (b << 1) | (((hi4 >> (8 * k)) & 0xffu) < cmp ? 1u : 0u);
        return b;
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) { // the pixel of tile row 4 band + j + 1
        const int gy = y0 + band * 4 + j;
        const uint32_t cmp = ct[j + 1];
        const uint32_t w = (row_bits(lo[j], hi[j], cmp) << 24) | (row_bits(lo[j + 2], hi[j + 2], cmp) << 16) |
                           (row_bits(lo[j + 3], hi[j + 3], cmp) << 8) | row_bits(lo[j + 4], hi[j + 4], cmp);
        if (gy < H) census[(size_t)gy * W + gx] = w;
    }
}

// the screened settings (stm_api.hip: packing_args_ok) as the kernels' source description
PackSrc make_src(const PackInput &in, int H, int W, int elem_sz)
{
    PackSrc s;
    const int axis = in.pk.packing >> 1, half = in.pk.packing & 1;
    s.p0 = in.nv12 ? in.y : in.frame;
    s.p1 = in.nv12 ? in.uv : nullptr;
    s.pitch0 = in.nv12 ? in.pitch_y : in.num_cols_sbs;
    s.pitch1 = in.nv12 ? in.pitch_uv : 0;
    s.elem_sz = elem_sz;
    s.n = axis == 0 ? (half ? W / 2 : W) : (half ? H / 2 : H);
    for (int e = 0; e < 2; ++e) s.org[e] = (e ^ in.pk.swap) * (s.n + in.pk.gap);
    s.c = PK_NV12_COEF[in.nv12 ? in.matrix : 0];
    return s;
}

// calls f.template run<FMT, AXIS, FILT>() for the input's format, axis and filter
template <class F> void dispatch(const PackInput &in, F f)
{
    const int axis = in.pk.packing >> 1, filt = (in.pk.packing & 1) ? 1 + in.pk.filter : 0;
    const int key = (in.nv12 ? 6 : 0) + axis * 3 + filt;
    switch (key) {
    case 0: f.template run<0, 0, 0>(); break;
    case 1: f.template run<0, 0, 1>(); break;
    case 2: f.template run<0, 0, 2>(); break;
    case 3: f.template run<0, 1, 0>(); break;
    case 4: f.template run<0, 1, 1>(); break;
    case 5: f.template run<0, 1, 2>(); break;
    case 6: f.template run<1, 0, 0>(); break;
    case 7: f.template run<1, 0, 1>(); break;
    case 8: f.template run<1, 0, 2>(); break;
    case 9: f.template run<1, 1, 0>(); break;
    case 10: f.template run<1, 1, 1>(); break;
    default: f.template run<1, 1, 2>(); break;
    }
}

struct DemuxLaunch {
    u8 *l, *r;
    PackSrc s;
    int H, W;
    template <int FMT, int AXIS, int FILT> void run() const
    {
        STM_LAUNCH((stm_k_demux_packed<FMT, AXIS, FILT>), dim3(cdiv(2 * W, 256), H), dim3(256), 0, stream(), l, r, s, W);
    }
};
struct FrontLaunch {
    u8 *l, *r;
    uint32_t *pk_l, *pk_r, *wide_l, *wide_r, *cen_l, *cen_r;
    PackSrc s;
    int H, W;
    template <int FMT, int AXIS, int FILT> void run() const
    {
        STM_LAUNCH((stm_k_front_pack<FMT, AXIS, FILT>), dim3(cdiv(W, PF_TX), cdiv(H, PF_TY), 2), dim3(256), 0, stream(), l, r, pk_l, pk_r,
                   wide_l, wide_r, cen_l, cen_r, s, H, W);
    }
};

} // namespace

void launch_demux_packed(u8 *l, u8 *r, const PackInput &in, int H, int W, int elem_sz)
{
    dispatch(in, DemuxLaunch{l, r, make_src(in, H, W, elem_sz), H, W});
    STM_CHECK_LAUNCH();
}

void launch_front_pack(u8 *l, u8 *r, uint32_t *pk_l, uint32_t *pk_r, uint32_t *wide_l, uint32_t *wide_r, uint32_t *cen_l, uint32_t *cen_r,
                       const PackInput &in, int H, int W, int elem_sz)
{
    ProfScope p("front_pack");
    dispatch(in, FrontLaunch{l, r, pk_l, pk_r, wide_l, wide_r, cen_l, cen_r, make_src(in, H, W, elem_sz), H, W});
    STM_CHECK_LAUNCH();
}

} // namespace stm
