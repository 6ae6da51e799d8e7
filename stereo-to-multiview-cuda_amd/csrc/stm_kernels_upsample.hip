// stm_kernels_upsample.hip -- guided disparity up-sampling for the reduced-resolution frame (joint bilateral upsampling, Kopf et
// al. 2007): a full-resolution map from the low-resolution one, each of its 4 x 4 low-resolution taps weighted by a tent in
// space and by how close the tap's colour in the LOW-resolution image is to the output pixel's colour in the FULL-resolution
// guide image.  A depth edge then lands on the colour edge of the image the views are rendered from instead of being smeared
// over a low-resolution pixel by the bilinear blend of stm_k_disp_scale.  An addition: the reference has no such step.
//
// Definition (include/stm_hip.h), f32 throughout, one operation per line, per output pixel (x, y):
//   xs, ys, x0, y0 as stm_k_disp_scale; taps (y0 + j, x0 + i), j, i = -1 .. 2 in ascending order, taps outside the low-resolution
//   image skipped; wy = fmaxf(0, 1 - fabsf(ys - yi) * 0.5f), wx alike; sad = |dB| + |dG| + |dR| of guide pixel and tap;
//   wgt = (wy * wx) * tab[sad]; sw += wgt; swd += wgt * dlow[tap]; out = (sw > 0 ? swd / sw : the bilinear value) * up.
//
// One kernel, stm_k_disp_upsample, for one or two views (blockIdx.z).  A block of 256 threads serves a tile of tw x th output
// pixels (64 x 4 unless the size ratio makes the footprint too large, see launch_disp_upsample), one pixel per lane, lanes along
// x, one output row per wave.  x0 and y0 are monotone in x and y, so the tile's taps are the rectangle between the first
// pixel's (x0 - 1, y0 - 1) and the last pixel's (x0 + 2, y0 + 2), clipped to the image: it is staged in LDS once, as one packed
// BGR0 dword and one f32 per low-resolution pixel (35 x 5 of them at ratio 2), next to the 766 colour weights.  A tap is then
// one ds_read_b64, one v_sad_u8 on the two packed pixels, one table read and five float operations.  The 16 taps are a
// fixed-trip unrolled loop; a tap outside the image reads a clamped slot and its contribution is predicated away (the rows are
// wave-uniform, so only the columns at the image's left and right edge diverge at all).  The clamped slots of taps (0, 0) ..
// (1, 1) are exactly the four values of the bilinear fallback, which is built from them in registers.
#include "stm_common.h"

namespace stm {

constexpr int UP_T = 256;    // threads per block: four waves, one output row each
constexpr int UP_TX = 64;    // widest tile (one wave along x)
constexpr int UP_TY = 4;     // tallest tile
constexpr int UP_CAP = 1024; // low-resolution pixels a block can stage (8 bytes each)
constexpr int UP_TAB = 766;  // colour weights: sad = 0 .. 3 * 255

struct UpsampleArgs { // both views of a frame share the launch
    float *out[2];
    const float *dlow[2];
    const u8 *ilow[2], *img[2];
};

// tx_disp_scale_kernel's own mapping of an output coordinate to the input (d_tx_scale.cu:15-18)
__device__ __forceinline__ float up_src(int o, int on, int in)
{
    float s = ((float)o / (float)on) * (float)in;
    return fminf(fmaxf(s, 0.0f), (float)(in - 1));
}

__global__ __launch_bounds__(UP_T) void stm_k_disp_upsample(UpsampleArgs a, const float *__restrict__ tab, int H, int W, int h, int w,
                                                            int elem_sz, float up, int tw, int th)
{
    __shared__ uint2 s_px[UP_CAP]; // .x = B | G << 8 | R << 16, .y = the disparity's bits
    __shared__ float s_tab[UP_TAB];
    const int v = blockIdx.z, tid = threadIdx.x, tx = tid & 63;
    const int ty = __builtin_amdgcn_readfirstlane(tid >> 6); // the wave's row, as a scalar: the row tests below branch, not mask
    float *__restrict__ out = a.out[v];
    const float *__restrict__ dlow = a.dlow[v];
    const u8 *__restrict__ ilow = a.ilow[v];
    const u8 *__restrict__ img = a.img[v];

    // ---- the tile and its footprint (block-uniform)
    const int X0 = blockIdx.x * tw, Y0 = blockIdx.y * th;
    const int X1 = min(X0 + tw, W) - 1, Y1 = min(Y0 + th, H) - 1;
    const int fx0 = max((int)floorf(up_src(X0, W, w)) - 1, 0), fx1 = min((int)floorf(up_src(X1, W, w)) + 2, w - 1);
    const int fy0 = max((int)floorf(up_src(Y0, H, h)) - 1, 0), fy1 = min((int)floorf(up_src(Y1, H, h)) + 2, h - 1);
    const int fw = fx1 - fx0 + 1, fh = fy1 - fy0 + 1; // fw * fh <= UP_CAP: launch_disp_upsample chose tw and th for it

    for (int k = tid; k < UP_TAB; k += UP_T) s_tab[k] = tab[k];
    for (int r = ty; r < fh; r += UP_T / 64) {
        const size_t grow = (size_t)(fy0 + r) * w + fx0;
        for (int c = tx; c < fw; c += 64) {
            const int slot = r * fw + c;
            const u8 *px = ilow + (grow + c) * elem_sz;
            const uint32_t bgr = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
            if (slot < UP_CAP) s_px[slot] = make_uint2(bgr, __float_as_uint(dlow[grow + c]));
        }
    }
    __syncthreads();

    const int x = X0 + tx, y = Y0 + ty;
    if (tx >= tw || ty >= th || x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const u8 *gp = img + p * elem_sz;
    const uint32_t guide = (uint32_t)gp[0] | ((uint32_t)gp[1] << 8) | ((uint32_t)gp[2] << 16);
    const float xs = up_src(x, W, w), ys = up_src(y, H, h);
    const int x0 = (int)floorf(xs), y0 = (int)floorf(ys);

    float sw = 0.0f, swd = 0.0f;
    float q[2][2]; // taps (0, 0) .. (1, 1) at their clamped positions: in[x0 | x1][y0 | y1] of stm_k_disp_scale
#pragma unroll
    for (int j = -1; j <= 2; ++j) {
        const int yi = y0 + j;
        const bool row_in = yi >= 0 && yi < h;
        const int rbase = (min(max(yi, 0), h - 1) - fy0) * fw - fx0;
        float wy = fabsf(ys - (float)yi) * 0.5f;
        wy = fmaxf(0.0f, 1.0f - wy);
#pragma unroll
        for (int i = -1; i <= 2; ++i) {
            const int xi = x0 + i;
            const bool in = row_in && xi >= 0 && xi < w;
            const int slot = min(rbase + min(max(xi, 0), w - 1), UP_CAP - 1);
            const uint2 e = s_px[slot];
            const float d = __uint_as_float(e.y);
            float wx = fabsf(xs - (float)xi) * 0.5f;
            wx = fmaxf(0.0f, 1.0f - wx);
            const uint32_t sad = __builtin_amdgcn_sad_u8(guide, e.x, 0u); // the fourth bytes are both 0
            const float wgt = (wy * wx) * s_tab[sad];
            const float t = wgt * d;
            if (in) { // a tap outside the image contributes nothing (not + 0: its clamped slot may hold anything)
                sw = sw + wgt;
                swd = swd + t;
            }
            if (j >= 0 && j <= 1 && i >= 0 && i <= 1) q[j][i] = d;
        }
    }
    // the value stm_k_disp_scale computes before its final multiplication, same lines, same order
    const float bx = xs - (float)x0, by = ys - (float)y0;
    float ta = q[0][0] * (1.0f - bx);
    float tb = q[0][1] * bx;
    const float top = ta + tb;
    ta = q[1][0] * (1.0f - bx);
    tb = q[1][1] * bx;
    const float bot = ta + tb;
    ta = top * (1.0f - by);
    tb = bot * by;
    const float bil = ta + tb;
    const float r = sw > 0.0f ? swd / sw : bil;
    out[p] = r * up;
}

// the low-resolution columns (rows) a tile of n output columns (rows) can touch, from above: x0 of the last pixel minus x0 of the
// first is at most floor(xs_last - xs_first) + 1, the two xs carry a rounding error far below 1 for in < 2^21, and the taps add
// one column before and two after
static int up_span(int n, int on, int in)
{
    const double s = floor((double)(n - 1) * (double)in / (double)on) + 6.0;
    return s < (double)in ? (int)s : in;
}

void launch_disp_upsample(int nviews, float *const *out, const float *const *dlow, const u8 *const *ilow, const u8 *const *img,
                          const float *tab, int H, int W, int h, int w, int elem_sz, float up)
{
    if (nviews < 1 || nviews > 2) {
        fail("launch_disp_upsample: 1 or 2 views", "nviews", __FILE__, __LINE__);
        return;
    }
    if (h >= (1 << 21) || w >= (1 << 21)) { // up_span's bound on the footprint
        fail("disp_upsample: more than 2^21 - 1 input rows or columns", "in_rows, in_cols", __FILE__, __LINE__);
        return;
    }
    // 64 x 4 output pixels per block while their taps fit the staging buffer (any ratio down to 2 / 3); a stronger reduction
    // takes a smaller tile (1 x 1 needs 4 x 4 taps: it always fits)
    int tw = UP_TX, th = UP_TY;
    while (up_span(tw, W, w) * up_span(th, H, h) > UP_CAP) {
        if (th > 1) th >>= 1;
        else tw >>= 1;
    }
    UpsampleArgs a;
    for (int v = 0; v < 2; ++v) {
        const int s = v < nviews ? v : 0;
        a.out[v] = out[s]; a.dlow[v] = dlow[s]; a.ilow[v] = ilow[s]; a.img[v] = img[s];
    }
    ProfScope p("upsample");
    STM_LAUNCH(stm_k_disp_upsample, dim3(cdiv(W, tw), cdiv(H, th), nviews), dim3(UP_T), 0, stream(), a, tab, H, W, h, w, elem_sz, up, tw,
               th);
    STM_CHECK_LAUNCH();
}

} // namespace stm
