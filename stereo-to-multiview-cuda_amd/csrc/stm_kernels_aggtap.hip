// stm_kernels_aggtap.hip -- the test tap on the frame's aggregation chain (stm_set_agg_tap, include/stm_hip.h): two copy kernels
// between the chain's own volume layouts and the caller's plain float [2][D][H][W].  Test access only: one thread per element,
// nothing tuned.  No aggregation kernel knows of the tap; with the tap off nothing here is launched.
#include "stm_common.h"

namespace stm {
namespace {

// float index of (true hypothesis d, row y, column x) inside one view's volume
//   TAP_PQ     float4 [d / 16][y][g][d % 16], pixel x = 4 g + k in component k (stm_kernels_aggm.hip)
//   TAP_PX     ((y 4G + x) 64 + L), the hypothesis d at float L of the pixel's record: L = d (order 0), 4 (d % 16) + d / 16 (order 1:
//              float L holds hypothesis 16 (L % 4) + L / 4), 16 (d % 4) + d / 4 (order 2: float 16 b + n holds 4 n + b); see px_order
//   TAP_QUADS  float4 [d / 4][y][x], the hypothesis d % 4 in component d % 4 (Vol::quad)
__device__ __forceinline__ size_t tap_index(int layout, int ord, int d, int y, int x, int H, int W, int G)
{
    if (layout == TAP_PQ) return ((((size_t)(d >> 4) * H + y) * G + (x >> 2)) * 16 + (d & 15)) * 4 + (x & 3);
    if (layout == TAP_PX) {
        const int L = ord == 0 ? d : ord == 1 ? 4 * (d & 15) + (d >> 4) : 16 * (d & 3) + (d >> 2);
        return ((size_t)y * 4 * G + x) * 64 + L;
    }
    return (((size_t)(d >> 2) * H + y) * W + x) * 4 + (d & 3);
}

// dst[view][d][y][x] = the volume's element, d < D, x < W; thread = one element of dst
__global__ __launch_bounds__(256) void stm_k_tap_read(const float *__restrict__ vol_l, const float *__restrict__ vol_r, float *__restrict__ dst,
                                                      int layout, int ord, int D, int H, int W, int G)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)D * H * W;
    if (i >= 2 * n) return;
    const int view = i >= n;
    const size_t e = i - (view ? n : 0);
    const int x = (int)(e % W), y = (int)(e / W % H), d = (int)(e / W / H);
    dst[i] = (view ? vol_r : vol_l)[tap_index(layout, ord, d, y, x, H, W, G)];
}

// the volume's elements d < D, x < W from src[view][d][y][x]; the padding hypotheses D <= d < Dpad of the layout's last chunk
// take -1.0f: no sum of costs is negative, so a last pass whose own d >= D guard is broken shows a winner outside the range.
// Columns x >= W of the padded layouts stay as they are.  thread = one element (view, d < Dpad, y, x)
__global__ __launch_bounds__(256) void stm_k_tap_write(float *__restrict__ vol_l, float *__restrict__ vol_r, const float *__restrict__ src,
                                                       int layout, int ord, int D, int Dpad, int H, int W, int G)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)Dpad * H * W;
    if (i >= 2 * n) return;
    const int view = i >= n;
    const size_t e = i - (view ? n : 0);
    const int x = (int)(e % W), y = (int)(e / W % H), d = (int)(e / W / H);
    const float val = d < D ? src[(((size_t)view * D + d) * H + y) * W + x] : -1.0f;
    (view ? vol_r : vol_l)[tap_index(layout, ord, d, y, x, H, W, G)] = val;
}

// hypotheses a volume of this layout stores per pixel: whole chunks of 16 (PQ; PX has exactly four), whole quads
int tap_dpad(int layout, int D) { return layout == TAP_QUADS ? (D + 3) / 4 * 4 : layout == TAP_PX ? 64 : (D + 15) / 16 * 16; }

} // namespace

void launch_tap_read(const float *vol_l, const float *vol_r, int layout, int ord, float *dst, int D, int H, int W)
{
    const size_t n = (size_t)2 * D * H * W;
    STM_LAUNCH(stm_k_tap_read, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream(), vol_l, vol_r, dst, layout, ord, D, H, W, (W + 3) / 4);
    STM_CHECK_LAUNCH();
}
void launch_tap_write(float *vol_l, float *vol_r, int layout, int ord, const float *src, int D, int H, int W)
{
    const int Dpad = tap_dpad(layout, D);
    const size_t n = (size_t)2 * Dpad * H * W;
    STM_LAUNCH(stm_k_tap_write, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream(), vol_l, vol_r, src, layout, ord, D, Dpad, H, W, (W + 3) / 4);
    STM_CHECK_LAUNCH();
}

} // namespace stm
