// stm_kernels_temporal.hip -- temporal stabilisation of the final disparity maps of a frame stream: a motion-adaptive recursive
// filter.  Where neither the colour around a pixel nor its disparity moved between two consecutive frames, the pixel's new
// disparity is pulled towards the one the previous frame put out; anywhere else it is left as matched.  An addition: the
// reference matches every frame of its video loop on its own.
//
// Definition (include/stm_hip.h), f32, one operation per line, per pixel p = (x, y):
//   sad(q) = |img[q][0] - img_prev[q][0]| + |..[1] - ..[1]| + |..[2] - ..[2]|;  m(p) = max of sad over the 3 x 3 pixels around p
//   that lie inside the H x W image;  c = cur[p];  q = prev[p];  t = q - c;  df = fabsf(t);
//   if (m(p) <= thresh_color && df <= thresh_disp) { u = alpha * t;  cur[p] = c + u; }
//
// One kernel, stm_k_disp_temporal, for one or two views (blockIdx.z).  A block of 256 threads serves a tile of 64 x 16 pixels,
// lanes along x, four rows per wave.  The block first computes sad once for every pixel of the tile and of its one-pixel halo
// (66 x 18) into LDS: two pixels packed to B | G << 8 | R << 16 (one dword load each where the pixels are four aligned bytes,
// three byte loads otherwise) and one v_sad_u8.  A halo pixel outside the image stores 0, which no maximum notices (every
// neighbourhood holds its own centre, and sad >= 0), so the clipped neighbourhood needs no test afterwards.  A thread then takes
// the horizontal maximum of three LDS entries for the six rows its four pixels touch (rows of 66 dwords read at lane, lane + 1,
// lane + 2: no bank conflicts) and folds three of them per pixel: 18 LDS reads for four pixels instead of 36.
//
// The images are addressed as base + offset + ((size_t)y * stride + x) * elem_sz with a row stride in pixels, so the frame
// hands over the two halves of the current and of the previous side-by-side buffer as they are.  x runs over the view's own W
// columns only: the neighbourhood of a pixel at the seam of the halves never reaches into the other half.
// A pixel is written only where the gate passes (`out = c` is what the map already holds).
#include "stm_common.h"

namespace stm {

constexpr int TP_T = 256;        // threads per block: four waves
constexpr int TP_TX = 64;        // tile width (one wave along x)
constexpr int TP_RPT = 4;        // rows per thread
constexpr int TP_TY = (TP_T / 64) * TP_RPT; // tile height
constexpr int TP_LW = TP_TX + 2, TP_LH = TP_TY + 2; // the tile with its halo

struct TemporalArgs { // both views of a frame share the launch
    float *cur[2];
    const float *prev[2];
    const u8 *img[2], *img_prev[2]; // the byte offsets of the views already applied
};

__device__ __forceinline__ uint32_t tp_pixel(const u8 *p, bool dword)
{
    if (dword) return *(const uint32_t *)p & 0xffffffu;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

__global__ __launch_bounds__(TP_T) void stm_k_disp_temporal(TemporalArgs a, int H, int W, int stride, int elem_sz, int dword, float alpha,
                                                            int thresh_color, float thresh_disp)
{
    __shared__ uint32_t s_sad[TP_LH][TP_LW];
    const int v = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float *__restrict__ cur = a.cur[v];
    const float *__restrict__ prev = a.prev[v];
    const u8 *__restrict__ img = a.img[v];
    const u8 *__restrict__ img_prev = a.img_prev[v];
    const int X0 = blockIdx.x * TP_TX, Y0 = blockIdx.y * TP_TY;

    // ---- sad of the tile and its halo, once per pixel
    for (int k = tid; k < TP_LH * TP_LW; k += TP_T) {
        const int r = k / TP_LW, c = k - r * TP_LW;
        const int gy = Y0 - 1 + r, gx = X0 - 1 + c;
        uint32_t s = 0u; // outside the image: takes no part in any maximum
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t o = ((size_t)gy * (size_t)stride + (size_t)gx) * (size_t)elem_sz;
            s = __builtin_amdgcn_sad_u8(tp_pixel(img + o, dword != 0), tp_pixel(img_prev + o, dword != 0), 0u); // the fourth bytes are both 0
        }
        s_sad[r][c] = s;
    }
    __syncthreads();

    // ---- horizontal maxima of the six rows this thread's four pixels touch, then three of them per pixel
    const int x = X0 + lane, r0 = wave * TP_RPT;
    uint32_t hm[TP_RPT + 2];
#pragma unroll
    for (int j = 0; j < TP_RPT + 2; ++j) hm[j] = max(max(s_sad[r0 + j][lane], s_sad[r0 + j][lane + 1]), s_sad[r0 + j][lane + 2]);
    if (x >= W) return;
#pragma unroll
    for (int j = 0; j < TP_RPT; ++j) {
        const int y = Y0 + r0 + j;
        if (y >= H) break;
        const int m = (int)max(max(hm[j], hm[j + 1]), hm[j + 2]);
        const size_t p = (size_t)y * W + x;
        const float c = cur[p];
        const float q = prev[p];
        const float t = q - c;
        const float df = fabsf(t);
        if (m <= thresh_color && df <= thresh_disp) { // a NaN in c or q fails the second test
            const float u = alpha * t;
            cur[p] = c + u;
        }
    }
}

void launch_disp_temporal(int nviews, float *const *cur, const float *const *prev, const u8 *const *img, const u8 *const *img_prev,
                          const size_t *byte_off, int H, int W, int stride, int elem_sz, float alpha, int thresh_color, float thresh_disp)
{
    if (nviews < 1 || nviews > 2) {
        fail("launch_disp_temporal: 1 or 2 views", "nviews", __FILE__, __LINE__);
        return;
    }
    if (H < 1 || W < 1 || stride < W || elem_sz < 3) { // the kernel's bounds rest on these
        fail("launch_disp_temporal: H, W >= 1, stride >= W, elem_sz >= 3", "H, W, stride, elem_sz", __FILE__, __LINE__);
        return;
    }
    TemporalArgs a;
    bool dword = elem_sz == 4; // a pixel is one aligned dword: every image address is base + 4 * k
    for (int v = 0; v < 2; ++v) {
        const int s = v < nviews ? v : 0;
        a.cur[v] = cur[s]; a.prev[v] = prev[s];
        a.img[v] = img[s] + byte_off[s]; a.img_prev[v] = img_prev[s] + byte_off[s];
        dword = dword && ((uintptr_t)a.img[v] & 3) == 0 && ((uintptr_t)a.img_prev[v] & 3) == 0;
    }
    ProfScope p("temporal");
    STM_LAUNCH(stm_k_disp_temporal, dim3(cdiv(W, TP_TX), cdiv(H, TP_TY), nviews), dim3(TP_T), 0, stream(), a, H, W, stride, elem_sz,
               dword ? 1 : 0, alpha, thresh_color, thresh_disp);
    STM_CHECK_LAUNCH();
}

} // namespace stm
