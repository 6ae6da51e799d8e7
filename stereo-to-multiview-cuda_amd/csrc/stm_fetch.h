// stm_fetch.h -- a pixel of an unpacked eye read straight from a frame call's input: BGR or NV12, any packing, or two images of their
// own.  Private to the kernels that run ahead of the front (stm_kernels_align.hip, stm_kernels_balance.hip, stm_kernels_cut.hip,
// stm_kernels_active.hip) and to the second eye of a packed 2D-plus-depth frame (stm_kernels_eye.hip, stm_k_eye_video).
// Everything has internal linkage, so each file compiles its own copy.
#pragma once
#include "stm_common.h"

namespace stm {

namespace {

// the gather, the filter and the conversion of stm_kernels_pack.hip, repeated because that file keeps them private (as it repeats
// stm_kernels_cost.hip's); the two eyes may come as two images of their own (the stage calls)
struct AlNv12Coef { int ky, rv, gu, gv, bu, yo; };
const AlNv12Coef AL_NV12_COEF[4] = {
    {76309, 104597, 25675, 53279, 132201, 16}, // 0: BT.601 limited range
    {76309, 117489, 13975, 34925, 138438, 16}, // 1: BT.709 limited range
    {65536, 91881, 22553, 46802, 116130, 0},   // 2: BT.601 full range
    {65536, 103206, 12276, 30679, 121609, 0},  // 3: BT.709 full range
};
__device__ __forceinline__ uint32_t al_nv12_bgrx(int Y, int U, int V, const AlNv12Coef &c)
{
    const int C = Y - c.yo, D = U - 128, E = V - 128, k = c.ky * C + 32768;
    const int b = min(max((k + c.bu * D) >> 16, 0), 255);
    const int g = min(max((k - c.gu * D - c.gv * E) >> 16, 0), 255);
    const int r = min(max((k + c.rv * E) >> 16, 0), 255);
    return (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16);
}
// p0[e]: the BGR frame or the Y plane eye e is read from, p1: the UV plane; pitch0 in pixels (BGR) or bytes (Y), pitch1 in bytes.
// org[e]: the first column (AXIS 0) or row (AXIS 1) of eye e, n: the packed eye's samples along the packing axis.
struct AlignSrc {
    const u8 *p0[2], *p1;
    int pitch0, pitch1, elem_sz;
    int org[2], n;
    AlNv12Coef c;
};
template <int FMT> __device__ __forceinline__ uint32_t al_frame_px(const AlignSrc &s, int e, int row, int col)
{
    if (FMT == 0) {
        const u8 *p = s.p0[e] + ((size_t)row * s.pitch0 + col) * s.elem_sz;
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
    const int Y = s.p0[e][(size_t)row * s.pitch0 + col];
    const u8 *q = s.p1 + (size_t)(row >> 1) * s.pitch1 + (col & ~1);
    return al_nv12_bgrx(Y, q[0], q[1], s.c);
}
template <int FMT, int AXIS> __device__ __forceinline__ uint32_t al_eye_px(const AlignSrc &s, int e, int i, int o)
{
    return AXIS == 0 ? al_frame_px<FMT>(s, e, o, s.org[e] + i) : al_frame_px<FMT>(s, e, s.org[e] + i, o);
}
__device__ __forceinline__ int al_clip255(int v) { return min(max(v, 0), 255); }
// FILT 0 = copy, 1 = linear, 2 = Catmull-Rom (stm_set_packing).  Pixel (x, y) of unpacked eye e, 0 <= x < W, 0 <= y < H.
template <int FMT, int AXIS, int FILT> __device__ __forceinline__ uint32_t al_unpacked_px(const AlignSrc &s, int e, int y, int x)
{
    const int a = AXIS == 0 ? x : y, o = AXIS == 0 ? y : x;
    if (FILT == 0) return al_eye_px<FMT, AXIS>(s, e, a, o);
    const int k = a >> 1, sg = (a & 1) ? 1 : -1, last = s.n - 1;
    const uint32_t p1 = al_eye_px<FMT, AXIS>(s, e, k, o), p2 = al_eye_px<FMT, AXIS>(s, e, min(max(k + sg, 0), last), o);
    uint32_t out = 0;
    if (FILT == 1) {
#pragma unroll
        for (int c = 0; c < 24; c += 8) {
            const int v = (96 * (int)((p1 >> c) & 0xff) + 32 * (int)((p2 >> c) & 0xff) + 64) >> 7;
            out |= (uint32_t)al_clip255(v) << c;
        }
        return out;
    }
    const uint32_t p0 = al_eye_px<FMT, AXIS>(s, e, min(max(k - sg, 0), last), o), p3 = al_eye_px<FMT, AXIS>(s, e, min(max(k + 2 * sg, 0), last), o);
#pragma unroll
    for (int c = 0; c < 24; c += 8) {
        const int v = (-9 * (int)((p0 >> c) & 0xff) + 111 * (int)((p1 >> c) & 0xff) + 29 * (int)((p2 >> c) & 0xff) -
                       3 * (int)((p3 >> c) & 0xff) + 64) >> 7;
        out |= (uint32_t)al_clip255(v) << c;
    }
    return out;
}

// the pair as the kernels take it: a screened frame (in != nullptr; stm_kernels_pack.hip's make_src), or two unpacked images
AlignSrc make_src(const PackInput *in, const u8 *img_l, const u8 *img_r, int H, int W, int elem_sz)
{
    AlignSrc s;
    s.elem_sz = elem_sz;
    if (!in) {
        s.p0[0] = img_l; s.p0[1] = img_r; s.p1 = nullptr;
        s.pitch0 = W; s.pitch1 = 0;
        s.org[0] = s.org[1] = 0;
        s.n = W;
        s.c = AL_NV12_COEF[0];
        return s;
    }
    const int axis = in->pk.packing >> 1, half = in->pk.packing & 1;
    s.p0[0] = s.p0[1] = in->nv12 ? in->y : in->frame;
    s.p1 = in->nv12 ? in->uv : nullptr;
    s.pitch0 = in->nv12 ? in->pitch_y : in->num_cols_sbs;
    s.pitch1 = in->nv12 ? in->pitch_uv : 0;
    s.n = axis == 0 ? (half ? W / 2 : W) : (half ? H / 2 : H);
    for (int e = 0; e < 2; ++e) s.org[e] = (e ^ in->pk.swap) * (s.n + in->pk.gap);
    s.c = AL_NV12_COEF[in->nv12 ? in->matrix : 0];
    return s;
}

// calls f.template run<FMT, AXIS, FILT>() for the input's format, axis and filter (two images: a plain BGR copy)
template <class F> void dispatch(const PackInput *in, F f)
{
    if (!in) { f.template run<0, 0, 0>(); return; }
    const int axis = in->pk.packing >> 1, filt = (in->pk.packing & 1) ? 1 + in->pk.filter : 0;
    switch ((in->nv12 ? 6 : 0) + axis * 3 + filt) {
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

} // namespace

} // namespace stm
