// stm_kernels_cost.hip -- AD-Census cost initialisation for gfx950 (wave64).
//
// Reference stages replaced:
//   mux_average_kernel        d_mux_common.cu:7-21     grey
//   tx_census_9x7_kernel_3    d_ci_census.cu:18-50     census transform
//   alu_hamdist_64            d_alu.cu:7-15            "Hamming" distance (low 32 bits, bit 31 weighs 33)
//   ci_ad_kernel_5            d_ci_ad.cu:73-159        absolute-difference cost
//   ci_census_kernel_6        d_ci_census.cu:197-254   census cost
//   ci_adcensus_kernel        d_ci_adcensus.cu:10-36   robust combine
// The reference materialises AD and census volumes (4 V of traffic) and combines them in a third
// pass; here one kernel writes the combined volume once.  Design notes:
//   * images are repacked once to one dword per pixel (B | G<<8 | R<<16): every later access is
//     a single aligned dword and |dB|+|dG|+|dR| is one v_sad_u8.
//   * alu_hamdist_64 only ever looks at the low 32 bits of the 48-bit census (int c = a ^ b), so
//     only that word (window rows y = -1, +1, +2, +3) is computed and stored.
//   * rho() is a table lookup (766 + 65 entries in LDS) -> results are bit-identical to the CPU.
#include "stm_common.h"

namespace stm {

// ---------------------------------------------------------------- pack BGR -> BGRX dword
__global__ __launch_bounds__(256) void stm_k_pack_bgrx(const u8 *__restrict__ bgr, uint32_t *__restrict__ packed,
                                                       int n, int elem_sz)
{
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u8 *p = bgr + (size_t)i * elem_sz;
    packed[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

void launch_pack_bgrx(const u8 *bgr, uint32_t *packed, int H, int W, int elem_sz)
{
    int n = H * W;
    STM_LAUNCH(stm_k_pack_bgrx, dim3(cdiv(n, 256)), dim3(256), 0, stream(), bgr, packed, n, elem_sz);
    STM_CHECK_LAUNCH();
}

// ---------------------------------------------------------------- grey + census (low word)
// grey = (u8)(b*c + g*c + r*c), three rounded products, left-to-right adds (d_mux_common.cu:16-20)
__device__ __forceinline__ uint32_t grey_of(uint32_t px)
{
    const float c = 0.33333334f;
    float b = (float)(px & 0xff) * c;
    float g = (float)((px >> 8) & 0xff) * c;
    float r = (float)((px >> 16) & 0xff) * c;
    float s = b + g;
    s = s + r;
    return (uint32_t)s;
}

constexpr int CEN_TX = 64, CEN_TY = 4;
// tile rows y0-1 .. y0+CEN_TY-1+3, cols x0-4 .. x0+CEN_TX-1+4, clamp-to-edge (d_ci_census.cu:39-40)
__global__ __launch_bounds__(CEN_TX *CEN_TY) void stm_k_census32(const uint32_t *__restrict__ packed_a,
                                                                uint32_t *__restrict__ census_a,
                                                                const uint32_t *__restrict__ packed_b,
                                                                uint32_t *__restrict__ census_b, int H, int W)
{
    const uint32_t *__restrict__ packed = blockIdx.z ? packed_b : packed_a; // blockIdx.z = view
    uint32_t *__restrict__ census = blockIdx.z ? census_b : census_a;
    constexpr int TW = CEN_TX + 8, TH = CEN_TY + 4;
    __shared__ u8 g[TH][TW + 4];
    int x0 = blockIdx.x * CEN_TX, y0 = blockIdx.y * CEN_TY;
    int tid = threadIdx.y * CEN_TX + threadIdx.x;
    for (int i = tid; i < TW * TH; i += CEN_TX * CEN_TY) {
        int ty = i / TW, tx = i - ty * TW;
        int gx = min(max(x0 + tx - 4, 0), W - 1);
        int gy = min(max(y0 + ty - 1, 0), H - 1);
        g[ty][tx] = (u8)grey_of(packed[(size_t)gy * W + gx]);
    }
    __syncthreads();
    int gx = x0 + threadIdx.x, gy = y0 + threadIdx.y;
    if (gx >= W || gy >= H) return;
    int cx = threadIdx.x + 4, cy = threadIdx.y + 1;
    uint32_t cmp = g[cy][cx];
    uint32_t w = 0;
    // bit order: y outer (-1, +1, +2, +3 survive the truncation to 32 bits), x inner -4..4 skipping 0,
    // appended MSB first (d_ci_census.cu:35-47)
    const int ys[4] = {-1, 1, 2, 3};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int x = -4; x <= 4; ++x) {
            if (x == 0) continue;
            w = (w << 1) | (g[cy + ys[j]][cx + x] < cmp ? 1u : 0u);
        }
    }
    census[(size_t)gy * W + gx] = w;
}

// both images of a pair in one launch
void launch_census32_pair(const uint32_t *packed_l, uint32_t *census_l, const uint32_t *packed_r, uint32_t *census_r, int H, int W)
{
    STM_LAUNCH(stm_k_census32, dim3(cdiv(W, CEN_TX), cdiv(H, CEN_TY), 2), dim3(CEN_TX, CEN_TY), 0, stream(),
                       packed_l, census_l, packed_r, census_r, H, W);
    STM_CHECK_LAUNCH();
}

// ---------------------------------------------------------------- frame pipeline: split + pixel formats + census
// stm_k_demux_sbs_packed and stm_k_census32 in one kernel: a block takes a 64 x 16 tile of one half of the side-by-side frame,
// reads it with the census halo (rows -1 .. +3, columns +-4) straight from the input, writes the three pixel formats of the
// tile's own pixels and keeps the grey values in LDS for the census word -- the BGRX plane is not read back, and 20 rows are
// loaded per 16 produced instead of 8 per 4.  A thread forms the census words of four consecutive rows of one column: their
// windows share eight tile rows, each read once as three dwords (nine grey bytes) instead of byte by byte.  The halo clamps to
// the edge of the block's OWN half (d_ci_census.cu:39-40 works on the split image): the left view's right border never sees the
// right view's first columns.  Requires Wsbs >= 2 W.
constexpr int FR_TX = 64, FR_TY = 16;
__global__ __launch_bounds__(256) void stm_k_front(u8 *__restrict__ l, u8 *__restrict__ r, uint32_t *__restrict__ pk_l, uint32_t *__restrict__ pk_r,
                                                   uint32_t *__restrict__ wide_l, uint32_t *__restrict__ wide_r, uint32_t *__restrict__ cen_l,
                                                   uint32_t *__restrict__ cen_r, const u8 *__restrict__ sbs, int H, int Wsbs, int W, int elem_sz)
{
    constexpr int TW = FR_TX + 8, TH = FR_TY + 4;
    __shared__ __attribute__((aligned(16))) u8 g[TH][TW + 4]; // (a row is 76 bytes: dword reads of a row stay aligned)
    const int view = blockIdx.z, x0 = blockIdx.x * FR_TX, y0 = blockIdx.y * FR_TY, tid = threadIdx.x;
    u8 *__restrict__ img = view ? r : l;
    uint32_t *__restrict__ pk = view ? pk_r : pk_l, *__restrict__ wide = view ? wide_r : wide_l, *__restrict__ census = view ? cen_r : cen_l;
    const u8 *__restrict__ half = sbs + (size_t)view * W * elem_sz;
    // All loads of a thread are issued before the first is used.  Own pixels: lane = column, wave w takes tile rows w, w + 4, ..
    // (a wave instruction = one 64-pixel row: aligned 256-byte stores of the dword formats); the 416 halo elements -- four full
    // rows, then eight side columns of the sixteen own rows -- take two more trips.
    const int lane = tid & 63, wave = tid >> 6;
    auto fetch = [&](int ty, int tx) {
        const int gx = min(max(x0 + tx - 4, 0), W - 1), gy = min(max(y0 + ty - 1, 0), H - 1); // clamp-to-edge inside this half
        const u8 *s = half + ((size_t)gy * Wsbs + gx) * elem_sz;
        return (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
    };
    constexpr int NH = TW * TH - FR_TX * FR_TY; // halo elements
    uint32_t own[FR_TY / 4], halo[2];
    int hty[2], htx[2];
#pragma unroll
    for (int k = 0; k < FR_TY / 4; ++k) own[k] = fetch(wave + 4 * k + 1, lane + 4);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int h = min(tid + 256 * m, NH - 1);
        if (h < 4 * TW) {
            const int q = h / TW;
            hty[m] = q == 0 ? 0 : FR_TY + q;
            htx[m] = h - q * TW;
        } else {
            const int e = h - 4 * TW;
            hty[m] = 1 + (e >> 3);
            htx[m] = (e & 7) < 4 ? (e & 7) : FR_TX + (e & 7);
        }
        halo[m] = fetch(hty[m], htx[m]);
    }
    // the split image as dwords: 64 pixels of 3 bytes are 48 aligned dwords of the row, each built from two neighbouring pixels
    const bool img_dwords = elem_sz == 3 && (W & 3) == 0 && x0 + FR_TX <= W && (((uintptr_t)img) & 3) == 0;
    const int p0 = (4 * lane) / 3, o8 = 8 * (4 * lane - 3 * p0); // lane < 48: dword `lane` starts in byte o8 / 8 of pixel p0
#pragma unroll
    for (int k = 0; k < FR_TY / 4; ++k) {
        const int r = wave + 4 * k, ux = x0 + lane, uy = y0 + r;
        g[r + 1][lane + 4] = (u8)grey_of(own[k]);
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
        if (tid + 256 * m < NH) g[hty[m]][htx[m]] = (u8)grey_of(halo[m]);
    __syncthreads();
    const int col = tid & 63, band = tid >> 6, gx = x0 + col; // rows y0 + 4 band .. + 3 of column gx
    if (gx >= W) return;
    // tile rows 4 band .. 4 band + 7, columns col .. col + 8 (the pixel's own column is col + 4): lo = the four bytes left of the
    // centre, ct = the centre, hi = the four bytes right of it
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
    // bit order of stm_k_census32: window rows -1, +1, +2, +3 (what survives the truncation to 32 bits), in a row x = -4 .. 4
    // without 0, appended MSB first (d_ci_census.cu:35-47)
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
void launch_front(u8 *l, u8 *r, uint32_t *pk_l, uint32_t *pk_r, uint32_t *wide_l, uint32_t *wide_r, uint32_t *cen_l, uint32_t *cen_r,
                  const u8 *sbs, int H, int Wsbs, int W, int elem_sz)
{
    ProfScope p("front"); // (host side only, and nothing at all unless stm_prof_enable: the yardstick of tools/overlay_time.py)
    STM_LAUNCH(stm_k_front, dim3(cdiv(W, FR_TX), cdiv(H, FR_TY), 2), dim3(256), 0, stream(), l, r, pk_l, pk_r, wide_l, wide_r, cen_l, cen_r,
               sbs, H, Wsbs, W, elem_sz);
    STM_CHECK_LAUNCH();
}

// ---------------------------------------------------------------- NV12 input: colour conversion in the same pass
// The integer conversion of stm_hip.h (stm_demux_nv12): 16.16 fixed point, 32-bit, arithmetic shift, no intermediate above 2^26.
// Row `matrix` of the table: ky, rv, gu, gv, bu (each round(coefficient * 65536)) and the luma offset.
struct Nv12Coef { int ky, rv, gu, gv, bu, yo; };
static const Nv12Coef NV12_COEF[4] = {
    {76309, 104597, 25675, 53279, 132201, 16}, // 0: BT.601 limited range
    {76309, 117489, 13975, 34925, 138438, 16}, // 1: BT.709 limited range
    {65536, 91881, 22553, 46802, 116130, 0},   // 2: BT.601 full range
    {65536, 103206, 12276, 30679, 121609, 0},  // 3: BT.709 full range
};
__device__ __forceinline__ uint32_t nv12_bgrx(int Y, int U, int V, const Nv12Coef &c)
{
    const int C = Y - c.yo, D = U - 128, E = V - 128, k = c.ky * C + 32768;
    const int b = min(max((k + c.bu * D) >> 16, 0), 255);
    const int g = min(max((k - c.gu * D - c.gv * E) >> 16, 0), 255);
    const int r = min(max((k + c.rv * E) >> 16, 0), 255);
    return (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16);
}
// stm_k_front on an NV12 frame: stm_k_front's tile, phase by phase and line by line (see there), with each pixel converted as it is
// fetched; from the converted BGRX dword on the two kernels are the same text.  (They do not share it through a device function:
// moving stm_k_front's body, or only its census phase, into an inlined function changed the ISA hipcc emits for stm_k_front, and
// the default path must not move -- DESIGN.md section 14.  Until the two are folded, DESIGN.md section 8 item 6, a change to
// stm_k_front's store or census phase must be repeated here by hand.)  A fetch is one Y byte and the pixel's U, V pair; hipcc merges the
// pair's two byte loads into one 16-bit load (gfx950 loads at any alignment), so a fetch issues two loads, as in stm_k_front.  The
// two lanes of a column pair read the same pair in the same instruction (one request to the cache), and the second tile row of a
// chroma row (another wave of the block: wave w keeps rows w, w + 4, .. so the store phase stays stm_k_front's) finds the line in
// the CU's vector cache: a chroma row of a tile is 64 bytes.
__global__ __launch_bounds__(256) void stm_k_front_nv12(u8 *__restrict__ l, u8 *__restrict__ r, uint32_t *__restrict__ pk_l,
                                                        uint32_t *__restrict__ pk_r, uint32_t *__restrict__ wide_l,
                                                        uint32_t *__restrict__ wide_r, uint32_t *__restrict__ cen_l,
                                                        uint32_t *__restrict__ cen_r, const u8 *__restrict__ yp, int pitch_y,
                                                        const u8 *__restrict__ uvp, int pitch_uv, int H, int W, int elem_sz, Nv12Coef c)
{
    constexpr int TW = FR_TX + 8, TH = FR_TY + 4;
    __shared__ __attribute__((aligned(16))) u8 g[TH][TW + 4]; // (a row is 76 bytes: dword reads of a row stay aligned)
    const int view = blockIdx.z, x0 = blockIdx.x * FR_TX, y0 = blockIdx.y * FR_TY, tid = threadIdx.x;
    u8 *__restrict__ img = view ? r : l;
    uint32_t *__restrict__ pk = view ? pk_r : pk_l, *__restrict__ wide = view ? wide_r : wide_l, *__restrict__ census = view ? cen_r : cen_l;
    const u8 *__restrict__ y_half = yp + (size_t)view * W, *__restrict__ uv_half = uvp + (size_t)view * W; // (W is even: a half starts on a chroma sample)
    // All loads of a thread are issued before the first is used.  Own pixels: lane = column, wave w takes tile rows w, w + 4, ..
    // (a wave instruction = one 64-pixel row: aligned 256-byte stores of the dword formats); the 416 halo elements -- four full
    // rows, then eight side columns of the sixteen own rows -- take two more trips.
    const int lane = tid & 63, wave = tid >> 6;
    auto fetch = [&](int ty, int tx) {
        const int gx = min(max(x0 + tx - 4, 0), W - 1), gy = min(max(y0 + ty - 1, 0), H - 1); // clamp-to-edge inside this half
        const int Y = y_half[(size_t)gy * pitch_y + gx];
        const u8 *s = uv_half + (size_t)(gy >> 1) * pitch_uv + (gx & ~1);
        return nv12_bgrx(Y, s[0], s[1], c);
    };
    constexpr int NH = TW * TH - FR_TX * FR_TY; // halo elements
    uint32_t own[FR_TY / 4], halo[2];
    int hty[2], htx[2];
#pragma unroll
    for (int k = 0; k < FR_TY / 4; ++k) own[k] = fetch(wave + 4 * k + 1, lane + 4);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int h = min(tid + 256 * m, NH - 1);
        if (h < 4 * TW) {
            const int q = h / TW;
            hty[m] = q == 0 ? 0 : FR_TY + q;
            htx[m] = h - q * TW;
        } else {
            const int e = h - 4 * TW;
            hty[m] = 1 + (e >> 3);
            htx[m] = (e & 7) < 4 ? (e & 7) : FR_TX + (e & 7);
        }
        halo[m] = fetch(hty[m], htx[m]);
    }
    // the split image as dwords: 64 pixels of 3 bytes are 48 aligned dwords of the row, each built from two neighbouring pixels
    const bool img_dwords = elem_sz == 3 && (W & 3) == 0 && x0 + FR_TX <= W && (((uintptr_t)img) & 3) == 0;
    const int p0 = (4 * lane) / 3, o8 = 8 * (4 * lane - 3 * p0); // lane < 48: dword `lane` starts in byte o8 / 8 of pixel p0
#pragma unroll
    for (int k = 0; k < FR_TY / 4; ++k) {
        const int r = wave + 4 * k, ux = x0 + lane, uy = y0 + r;
        g[r + 1][lane + 4] = (u8)grey_of(own[k]);
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
        if (tid + 256 * m < NH) g[hty[m]][htx[m]] = (u8)grey_of(halo[m]);
    __syncthreads();
    const int col = tid & 63, band = tid >> 6, gx = x0 + col; // rows y0 + 4 band .. + 3 of column gx
    if (gx >= W) return;
    // tile rows 4 band .. 4 band + 7, columns col .. col + 8 (the pixel's own column is col + 4): lo = the four bytes left of the
    // centre, ct = the centre, hi = the four bytes right of it
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
    // bit order of stm_k_census32: window rows -1, +1, +2, +3 (what survives the truncation to 32 bits), in a row x = -4 .. 4
    // without 0, appended MSB first (d_ci_census.cu:35-47)
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
void launch_front_nv12(u8 *l, u8 *r, uint32_t *pk_l, uint32_t *pk_r, uint32_t *wide_l, uint32_t *wide_r, uint32_t *cen_l, uint32_t *cen_r,
                       const u8 *y, int pitch_y, const u8 *uv, int pitch_uv, int H, int W, int elem_sz, int matrix)
{
    STM_LAUNCH(stm_k_front_nv12, dim3(cdiv(W, FR_TX), cdiv(H, FR_TY), 2), dim3(256), 0, stream(), l, r, pk_l, pk_r, wide_l, wide_r, cen_l, cen_r,
               y, pitch_y, uv, pitch_uv, H, W, elem_sz, NV12_COEF[matrix]);
    STM_CHECK_LAUNCH();
}
// the plain converter + split (stm_demux_nv12, and the frame under stm_set_agg_variant(600)): one thread per pixel of the two halves,
// no derived planes
__global__ __launch_bounds__(256) void stm_k_demux_nv12(u8 *__restrict__ l, u8 *__restrict__ r, const u8 *__restrict__ yp, int pitch_y,
                                                        const u8 *__restrict__ uvp, int pitch_uv, int W, int elem_sz, Nv12Coef c)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= 2 * W) return;
    const u8 *s = uvp + (size_t)(y >> 1) * pitch_uv + (x & ~1);
    const uint32_t px = nv12_bgrx(yp[(size_t)y * pitch_y + x], s[0], s[1], c);
    const bool right = x >= W;
    u8 *d = (right ? r : l) + ((size_t)y * W + (right ? x - W : x)) * elem_sz;
    d[0] = (u8)px; d[1] = (u8)(px >> 8); d[2] = (u8)(px >> 16);
}
void launch_demux_nv12(u8 *l, u8 *r, const u8 *y, int pitch_y, const u8 *uv, int pitch_uv, int H, int W, int elem_sz, int matrix)
{
    STM_LAUNCH(stm_k_demux_nv12, dim3(cdiv(2 * W, 256), H), dim3(256), 0, stream(), l, r, y, pitch_y, uv, pitch_uv, W, elem_sz,
               NV12_COEF[matrix]);
    STM_CHECK_LAUNCH();
}

// ---------------------------------------------------------------- reduced-resolution frame: split + reduction + pixel formats + census
// Everything the reduced frame needs before frame_disparity, in one launch.  The grid is one list of 64 x 16 tiles: rows
// blockIdx.y < nty are tiles of the REDUCED image (h x w), the rows after them tiles of the full-size split image (H x W);
// blockIdx.z = view.  The branch between the two is uniform for the block.
//   A reduced tile is stm_k_front's tile, phase by phase and line by line (see there), with one difference: a `fetch` does not read
// a pixel of the frame but computes a pixel of the reduced image -- stm_k_scale_bilinear's arithmetic (tx_scale_bilinear_kernel,
// d_tx_scale.cu:30-52, and bilinear_u8: the same f32 operations in the same order, its clamps) on four taps read straight from
// the input frame.  The taps clamp to the last column and row of the block's OWN eye, as the scale kernel does on the split image;
// the halo clamps to the reduced image's edge BEFORE the pixel is computed, as stm_k_census32 does on the reduced image.  So the
// low image, the three derived planes and the census words are bit for bit those of the unfused chain (demux, scale, pack,
// census32), and the reduced image is never read back.
//   A split tile copies (NV12: converts) its 64 x 16 pixels of one eye into the full-size image the renderer, the guided
// up-sampler and the temporal step read, with stm_k_front's dword stores.
//   SRC: where a tap comes from.  BGR: p0 = the side-by-side frame, pitch0 = its pixels a row.  NV12: p0 / p1 = the Y / UV planes,
// pitch0 / pitch1 their bytes a row, a tap is nv12_bgrx of its samples -- so the reduced image is the reduction of the CONVERTED
// split image.  Any h, w >= 1: w < 9 (the halo is wider than the image), h >= H (ratio 1, up-scaling), elem_sz > 3.
struct LowSrc {
    const u8 *p0, *p1;
    int pitch0, pitch1;
    Nv12Coef c;
};
template <bool NV12>
__device__ __forceinline__ uint32_t low_src_px(const LowSrc &s, int view, int W, int elem_sz, int x, int y) // 0 <= x < W, 0 <= y < H
{
    if (NV12) {
        const int X = view * W + x; // (W is even: a half starts on a chroma sample)
        const int Y = s.p0[(size_t)y * s.pitch0 + X];
        const u8 *q = s.p1 + (size_t)(y >> 1) * s.pitch1 + (X & ~1);
        return nv12_bgrx(Y, q[0], q[1], s.c);
    }
    const u8 *q = s.p0 + ((size_t)y * s.pitch0 + (size_t)view * W + x) * elem_sz;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
}
// bilinear_u8 (stm_kernels_dibr.hip) on the three channels of four BGRX taps
__device__ __forceinline__ uint32_t bilinear_bgrx(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, float wx, float wy)
{
    uint32_t o = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float v00 = (float)((p00 >> (8 * ch)) & 0xffu), v01 = (float)((p01 >> (8 * ch)) & 0xffu);
        const float v10 = (float)((p10 >> (8 * ch)) & 0xffu), v11 = (float)((p11 >> (8 * ch)) & 0xffu);
        float a = v00 * (1.0f - wx);
        float b = v01 * wx;
        const float top = a + b;
        a = v10 * (1.0f - wx);
        b = v11 * wx;
        const float bot = a + b;
        a = top * (1.0f - wy);
        b = bot * wy;
        o |= (uint32_t)(u8)(a + b) << (8 * ch);
    }
    return o;
}
template <bool NV12>
__global__ __launch_bounds__(256) void stm_k_front_low(u8 *__restrict__ l, u8 *__restrict__ r, u8 *__restrict__ low_l, u8 *__restrict__ low_r,
                                                       uint32_t *__restrict__ pk_l, uint32_t *__restrict__ pk_r, uint32_t *__restrict__ wide_l,
                                                       uint32_t *__restrict__ wide_r, uint32_t *__restrict__ cen_l, uint32_t *__restrict__ cen_r,
                                                       LowSrc src, int H, int W, int h, int w, int elem_sz, int ntx, int nty, int stx)
{
    constexpr int TW = FR_TX + 8, TH = FR_TY + 4;
    __shared__ __attribute__((aligned(16))) u8 g[TH][TW + 4]; // (a row is 76 bytes: dword reads of a row stay aligned)
    const int view = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = (4 * lane) / 3, o8 = 8 * (4 * lane - 3 * p0); // lane < 48: dword `lane` starts in byte o8 / 8 of pixel p0
    if ((int)blockIdx.y >= nty) { // ---- a tile of the full-size split image
        if ((int)blockIdx.x >= stx) return;
        const int x0 = blockIdx.x * FR_TX, y0 = ((int)blockIdx.y - nty) * FR_TY;
        u8 *__restrict__ img = view ? r : l;
        uint32_t own[FR_TY / 4];
#pragma unroll
        for (int k = 0; k < FR_TY / 4; ++k) own[k] = low_src_px<NV12>(src, view, W, elem_sz, min(x0 + lane, W - 1), min(y0 + wave + 4 * k, H - 1));
        const bool img_dwords = elem_sz == 3 && (W & 3) == 0 && x0 + FR_TX <= W && (((uintptr_t)img) & 3) == 0;
#pragma unroll
        for (int k = 0; k < FR_TY / 4; ++k) {
            const int ux = x0 + lane, uy = y0 + wave + 4 * k;
            if (uy >= H) continue; // (the whole wave)
            if (img_dwords) {
                const uint32_t lo = (uint32_t)__shfl((int)own[k], p0 & 63), hi = (uint32_t)__shfl((int)own[k], (p0 + 1) & 63);
                if (lane < 48) ((uint32_t *)(img + ((size_t)uy * W + x0) * 3))[lane] = (uint32_t)((lo | ((unsigned long long)hi << 24)) >> o8);
            } else if (ux < W) {
                u8 *d = img + ((size_t)uy * W + ux) * elem_sz;
                d[0] = (u8)own[k]; d[1] = (u8)(own[k] >> 8); d[2] = (u8)(own[k] >> 16);
            }
        }
        return;
    }
    // ---- a tile of the reduced image
    if ((int)blockIdx.x >= ntx) return;
    const int x0 = blockIdx.x * FR_TX, y0 = blockIdx.y * FR_TY;
    u8 *__restrict__ img = view ? low_r : low_l;
    uint32_t *__restrict__ pk = view ? pk_r : pk_l, *__restrict__ wide = view ? wide_r : wide_l, *__restrict__ census = view ? cen_r : cen_l;
    const float fw = (float)w, fh = (float)h, fW = (float)W, fH = (float)H;
    auto fetch = [&](int ty, int tx) {
        const int gx = min(max(x0 + tx - 4, 0), w - 1), gy = min(max(y0 + ty - 1, 0), h - 1); // clamp-to-edge of the reduced image
        float xs = ((float)gx / fw) * fW;
        xs = fminf(fmaxf(xs, 0.0f), (float)(W - 1));
        float ys = ((float)gy / fh) * fH;
        ys = fminf(fmaxf(ys, 0.0f), (float)(H - 1));
        const int sx0 = (int)floorf(xs), sy0 = (int)floorf(ys); // in 0 .. W - 1, 0 .. H - 1: xs, ys were clamped
        const int sx1 = min(sx0 + 1, W - 1), sy1 = min(sy0 + 1, H - 1); // inside this eye, never the other half
        const float wx = xs - (float)sx0, wy = ys - (float)sy0;
        return bilinear_bgrx(low_src_px<NV12>(src, view, W, elem_sz, sx0, sy0), low_src_px<NV12>(src, view, W, elem_sz, sx1, sy0),
                             low_src_px<NV12>(src, view, W, elem_sz, sx0, sy1), low_src_px<NV12>(src, view, W, elem_sz, sx1, sy1), wx, wy);
    };
    // own pixels: lane = column, wave w takes tile rows w, w + 4, ..; the 416 halo elements -- four full rows, then eight side
    // columns of the sixteen own rows -- take two more trips (stm_k_front)
    constexpr int NH = TW * TH - FR_TX * FR_TY; // halo elements
    uint32_t own[FR_TY / 4], halo[2];
    int hty[2], htx[2];
#pragma unroll
    for (int k = 0; k < FR_TY / 4; ++k) own[k] = fetch(wave + 4 * k + 1, lane + 4);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int e0 = min(tid + 256 * m, NH - 1);
        if (e0 < 4 * TW) {
            const int q = e0 / TW;
            hty[m] = q == 0 ? 0 : FR_TY + q;
            htx[m] = e0 - q * TW;
        } else {
            const int e = e0 - 4 * TW;
            hty[m] = 1 + (e >> 3);
            htx[m] = (e & 7) < 4 ? (e & 7) : FR_TX + (e & 7);
        }
        halo[m] = fetch(hty[m], htx[m]);
    }
    // the reduced image as dwords: 64 pixels of 3 bytes are 48 aligned dwords of the row, each built from two neighbouring pixels
    const bool img_dwords = elem_sz == 3 && (w & 3) == 0 && x0 + FR_TX <= w && (((uintptr_t)img) & 3) == 0;
#pragma unroll
    for (int k = 0; k < FR_TY / 4; ++k) {
        const int rr0 = wave + 4 * k, ux = x0 + lane, uy = y0 + rr0;
        g[rr0 + 1][lane + 4] = (u8)grey_of(own[k]);
        if (uy >= h) continue; // (the whole wave)
        const uint32_t b = own[k] & 0xff, gg = (own[k] >> 8) & 0xff, rr = own[k] >> 16;
        const size_t p = (size_t)uy * w + ux;
        if (img_dwords) {
            const uint32_t lo = (uint32_t)__shfl((int)own[k], p0 & 63), hi = (uint32_t)__shfl((int)own[k], (p0 + 1) & 63);
            if (lane < 48) ((uint32_t *)(img + ((size_t)uy * w + x0) * 3))[lane] = (uint32_t)((lo | ((unsigned long long)hi << 24)) >> o8);
        } else if (ux < w) {
            u8 *d = img + p * elem_sz;
            d[0] = (u8)b; d[1] = (u8)gg; d[2] = (u8)rr;
        }
        if (ux < w) {
            pk[p] = own[k];
            wide[p] = b | (gg << 10) | (rr << 20);
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
        if (tid + 256 * m < NH) g[hty[m]][htx[m]] = (u8)grey_of(halo[m]);
    __syncthreads();
    const int col = tid & 63, band = tid >> 6, gx = x0 + col; // rows y0 + 4 band .. + 3 of column gx
    if (gx >= w) return;
    // tile rows 4 band .. 4 band + 7, columns col .. col + 8 (the pixel's own column is col + 4): lo = the four bytes left of the
    // centre, ct = the centre, hi = the four bytes right of it
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
    // bit order of stm_k_census32: window rows -1, +1, +2, +3 (what survives the truncation to 32 bits), in a row x = -4 .. 4
    // without 0, appended MSB first (d_ci_census.cu:35-47)
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
        const uint32_t wd = (row_bits(lo[j], hi[j], cmp) << 24) | (row_bits(lo[j + 2], hi[j + 2], cmp) << 16) |
                            (row_bits(lo[j + 3], hi[j + 3], cmp) << 8) | row_bits(lo[j + 4], hi[j + 4], cmp);
        if (gy < h) census[(size_t)gy * w + gx] = wd;
    }
}
// sbs != nullptr: a side-by-side BGR frame of Wsbs >= 2 W pixels a row; otherwise NV12 planes (y, uv, their pitches, matrix), all
// screened by the caller.  l / r: H x W x elem_sz, low_l / low_r: h x w x elem_sz, the six planes: h x w dwords
void launch_front_low(u8 *l, u8 *r, u8 *low_l, u8 *low_r, uint32_t *pk_l, uint32_t *pk_r, uint32_t *wide_l, uint32_t *wide_r, uint32_t *cen_l,
                      uint32_t *cen_r, const u8 *sbs, int Wsbs, const u8 *y, int pitch_y, const u8 *uv, int pitch_uv, int matrix, int H, int W,
                      int h, int w, int elem_sz)
{
    const int ntx = cdiv(w, FR_TX), nty = cdiv(h, FR_TY), stx = cdiv(W, FR_TX), sty = cdiv(H, FR_TY);
    const dim3 grid(ntx > stx ? ntx : stx, nty + sty, 2);
    if (sbs) {
        const LowSrc src = {sbs, nullptr, Wsbs, 0, NV12_COEF[0]};
        STM_LAUNCH(stm_k_front_low<false>, grid, dim3(256), 0, stream(), l, r, low_l, low_r, pk_l, pk_r, wide_l, wide_r, cen_l, cen_r, src, H, W,
                   h, w, elem_sz, ntx, nty, stx);
    } else {
        const LowSrc src = {y, uv, pitch_y, pitch_uv, NV12_COEF[matrix]};
        STM_LAUNCH(stm_k_front_low<true>, grid, dim3(256), 0, stream(), l, r, low_l, low_r, pk_l, pk_r, wide_l, wide_r, cen_l, cen_r, src, H, W,
                   h, w, elem_sz, ntx, nty, stx);
    }
    STM_CHECK_LAUNCH();
}

// ---------------------------------------------------------------- combined cost volume
// popc(x & 0x7fffffff) + 33 * (x >> 31)  ==  the 64-iteration loop of d_alu.cu:7-15 (SURVEY A-Q1)
__device__ __forceinline__ int hamdist_ref(uint32_t a, uint32_t b)
{
    uint32_t x = a ^ b;
    return __popc(x & 0x7fffffffu) + 33 * (int)(x >> 31);
}

constexpr int CI_TX = 256;
// one block = CI_TX pixels of one row, all D hypotheses.
// left  cost: L(x) vs R(clamp(x + o)), right cost: R(x) vs L(clamp(x - o)), o = d - zd  (A-Q6, clean A-Q7)
template <bool QUAD>
__global__ __launch_bounds__(CI_TX) void stm_k_cost_init(const uint32_t *__restrict__ pk_l, const uint32_t *__restrict__ pk_r,
                                                         const uint32_t *__restrict__ cen_l, const uint32_t *__restrict__ cen_r,
                                                         Vol cost_l, Vol cost_r,
                                                         const float *__restrict__ lut_ad_g, const float *__restrict__ lut_census_g,
                                                         int D, int zd, int H, int W, int pad)
{
    extern __shared__ uint32_t sm[];
    const int span = CI_TX + 2 * pad;
    uint32_t *s_pl = sm, *s_pr = sm + span, *s_cl = sm + 2 * span, *s_cr = sm + 3 * span;
    float *s_lut_ad = (float *)(sm + 4 * span);
    float *s_lut_c = s_lut_ad + 768;

    int y = blockIdx.y, x0 = blockIdx.x * CI_TX, tid = threadIdx.x;
    size_t row = (size_t)y * W;
    for (int i = tid; i < span; i += CI_TX) {
        int gx = min(max(x0 + i - pad, 0), W - 1);
        s_pl[i] = pk_l[row + gx];
        s_pr[i] = pk_r[row + gx];
        s_cl[i] = cen_l[row + gx];
        s_cr[i] = cen_r[row + gx];
    }
    for (int i = tid; i < 766; i += CI_TX) s_lut_ad[i] = lut_ad_g[i];
    if (tid < 65) s_lut_c[tid] = lut_census_g[tid];
    __syncthreads();

    int x = x0 + tid;
    if (x >= W) return;
    int c = tid + pad;
    uint32_t pl0 = s_pl[c], pr0 = s_pr[c], cl0 = s_cl[c], cr0 = s_cr[c];
    const int nq = (D + 3) >> 2;
    for (int q = 0; q < nq; ++q) {
        float vl[4], vr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = q * 4 + j;
            vl[j] = 0.f;
            vr[j] = 0.f;
            if (d < D) {
                const int o = d - zd;
                // clamp-to-edge is in GLOBAL coordinates; the tile was filled with clamped pixels, so a plain
                // tile offset reproduces it as long as |o| <= pad (pad = max(zd, D-1-zd)).
                uint32_t pr1 = s_pr[c + o], cr1 = s_cr[c + o];
                uint32_t pl1 = s_pl[c - o], cl1 = s_cl[c - o];
                int ad_l = (int)__builtin_amdgcn_sad_u8(pl0, pr1, 0u);
                int ad_r = (int)__builtin_amdgcn_sad_u8(pr0, pl1, 0u);
                int h_l = hamdist_ref(cl0, cr1);
                int h_r = hamdist_ref(cr0, cl1);
                vl[j] = s_lut_ad[ad_l] + s_lut_c[h_l];
                vr[j] = s_lut_ad[ad_r] + s_lut_c[h_r];
            }
        }
        store_quad<QUAD, false>(cost_l, q, D, row + x, make_float4(vl[0], vl[1], vl[2], vl[3]));
        store_quad<QUAD, false>(cost_r, q, D, row + x, make_float4(vr[0], vr[1], vr[2], vr[3]));
    }
}

void launch_cost_init(const uint32_t *pk_l, const uint32_t *pk_r, const uint32_t *cen_l, const uint32_t *cen_r,
                      Vol cost_l, Vol cost_r, const float *lut_ad, const float *lut_census,
                      int D, int zd, int H, int W)
{
    int pad = zd > D - 1 - zd ? zd : D - 1 - zd;
    if (pad < 0) pad = 0;
    size_t smem = (size_t)(4 * (CI_TX + 2 * pad) + 768 + 72) * 4;
    ProfScope p("cost_init");
    if (cost_l.quad)
        STM_LAUNCH(stm_k_cost_init<true>, dim3(cdiv(W, CI_TX), H), dim3(CI_TX), smem, stream(),
                           pk_l, pk_r, cen_l, cen_r, cost_l, cost_r, lut_ad, lut_census, D, zd, H, W, pad);
    else
        STM_LAUNCH(stm_k_cost_init<false>, dim3(cdiv(W, CI_TX), H), dim3(CI_TX), smem, stream(),
                           pk_l, pk_r, cen_l, cen_r, cost_l, cost_r, lut_ad, lut_census, D, zd, H, W, pad);
    STM_CHECK_LAUNCH();
}

// ref_quirks (stm_set_ref_quirks, non-default; SURVEY A-Q7): the reference's live kernels read one element past their shared
// tiles at d = 0 in two columns of every block of 160 -- the left cost of tx = 0 pairs L(x) with census_l / img_l at
// clamp(x + 160 + zd - 2) (the last element of the LEFT tile, d_ci_census.cu:240-246 with the padding of d_ci_adcensus.cu:117-120),
// the right cost of tx = 159 pairs R(x) with census_r / img_r at clamp(x - 158 - zd) (the first element of the right tile);
// the AD term strays only when D - zd <= zd (d_ci_adcensus.cu:57-59, d_ci_ad.cu:133-144).  This kernel overwrites those
// entries of plane 0 after stm_k_cost_init wrote the clean costs.  One thread per (row, block of 160, side).
__global__ __launch_bounds__(256) void stm_k_cost_quirks(const uint32_t *__restrict__ pk_l, const uint32_t *__restrict__ pk_r,
                                                         const uint32_t *__restrict__ cen_l, const uint32_t *__restrict__ cen_r,
                                                         Vol cost_l, Vol cost_r, const float *__restrict__ lut_ad,
                                                         const float *__restrict__ lut_c, int D, int zd, int H, int W, int nblk)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= H * nblk * 2) return;
    const int side = t & 1, b = (t >> 1) % nblk, y = (t >> 1) / nblk;
    const int x = b * 160 + (side ? 159 : 0);
    if (x >= W) return;
    const size_t row = (size_t)y * W;
    const bool ad_stray = (D - zd) <= zd;
    const uint32_t *pk_own = side ? pk_r : pk_l, *cen_own = side ? cen_r : cen_l;
    const int xs = min(max(side ? x - 158 - zd : x + 160 + zd - 2, 0), W - 1); // the stray element, in the OWN image
    const int xc = min(max(side ? x + zd : x - zd, 0), W - 1);                   // the clean partner at d = 0, in the other image
    const uint32_t p_other = ad_stray ? pk_own[row + xs] : (side ? pk_l : pk_r)[row + xc];
    const int ad = (int)__builtin_amdgcn_sad_u8(pk_own[row + x], p_other, 0u);
    const int hd = hamdist_ref(cen_own[row + x], cen_own[row + xs]);
    const float c = lut_ad[ad] + lut_c[hd];
    const Vol &dst = side ? cost_r : cost_l;
    if (dst.quad) ((float *)dst.base)[((size_t)0 * dst.plane_stride + row + x) * 4] = c; // hypothesis 0 of quad 0
    else dst.plane(0)[row + x] = c;
}

void launch_cost_quirks(const uint32_t *pk_l, const uint32_t *pk_r, const uint32_t *cen_l, const uint32_t *cen_r, Vol cost_l,
                        Vol cost_r, const float *lut_ad, const float *lut_census, int D, int zd, int H, int W)
{
    const int nblk = cdiv(W, 160), n = H * nblk * 2;
    STM_LAUNCH(stm_k_cost_quirks, dim3(cdiv(n, 256)), dim3(256), 0, stream(), pk_l, pk_r, cen_l, cen_r, cost_l, cost_r, lut_ad,
               lut_census, D, zd, H, W, nblk);
    STM_CHECK_LAUNCH();
}

} // namespace stm
