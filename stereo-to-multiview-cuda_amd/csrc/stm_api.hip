// stm_api.hip -- the C ABI (include/stm_hip.h): host-flavour and device-flavour stage entry points
// and the device-resident frame pipeline.  Mirrors the reference's per-stage host API
// (SURVEY.md section 8b); each function cites the reference wrapper it replaces.
#include "stm_common.h"
#include <initializer_list>
#include <mutex>
#include "../../include/stm_hip.h"
#include "../../include/stm_rectify.h"
#include "../../include/stm_hslo_tap.h"

#include <map>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <tuple>
#include <vector>

using namespace stm;

namespace {

// ---------------------------------------------------------------- small persistent device tables
struct DevTable {
    float *d = nullptr;
    size_t n = 0;
};
std::map<std::tuple<int, int, float, float>, DevTable> g_tables; // (dev*8+kind, size/radius, p0, p1)

int cur_dev()
{
    int dev = 0;
    STM_CHECK(hipGetDevice(&dev));
    return dev;
}

const float *dev_table(int kind, int size, float p0, float p1, size_t n, void (*fill)(float *, int, float, float))
{
    static std::mutex mu; // tables are shared by all host threads of the process
    std::lock_guard<std::mutex> lock(mu);
    auto key = std::make_tuple(cur_dev() * 8 + kind, size, p0, p1);
    auto it = g_tables.find(key);
    if (it != g_tables.end()) return it->second.d;
    std::vector<float> h(n);
    fill(h.data(), size, p0, p1);
    DevTable t;
    t.n = n;
    STM_CHECK(hipMalloc((void **)&t.d, n * sizeof(float)));
    STM_CHECK(hipMemcpy(t.d, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    g_tables[key] = t;
    return t.d;
}
void fill_rho(float *h, int, float ad, float ce) { rho_luts(ad, ce, h, h + 768); }
void fill_g2(float *h, int r, float s, float) { gaussian_kernel_2d(h, r, s); }
void fill_g1(float *h, int n, float s, float) { gaussian_kernel_1d(h, n, s); }

const float *rho_table(float ad, float ce) { return dev_table(0, 0, ad, ce, 768 + 72, fill_rho); } // [0..765] ad, [768..832] census
const float *gauss2d_table(int r, float s) { return dev_table(1, r, s, 0.f, (size_t)(2 * r + 1) * (2 * r + 1), fill_g2); }
const float *gauss1d_table(int n, float s) { return dev_table(2, n, s, 0.f, (size_t)(n > 0 ? n : 1), fill_g1); }
// the colour weights of the guided up-sampler (stm_hip.h): entry s = exp(-s^2 / (2 sigma^2)) in double, rounded once, s = 0 .. 765
void fill_up(float *h, int, float sigma, float)
{
    for (int s = 0; s < 766; ++s) h[s] = (float)exp(-(double)(s * s) / (2.0 * (double)sigma * (double)sigma));
}
const float *upsample_table(float sigma_color) { return dev_table(4, 0, sigma_color, 0.f, 768, fill_up); }
// The radius-7 bilateral filter of a map that holds ONE whole number c in a pixel's whole 15 x 15 neighbourhood: every tap has the
// weight spatial x colour[0], and the pixel's result is the same sequence of float operations whatever the pixel
// (d_filter_bilateral.cu:284-300: weight = spatial * colour, norm += weight, res += value * weight, res / norm) -- a function of c
// alone.  Entry i = the result for c = i - zd (the values a disparity map of this frame can hold), computed here with the kernel's
// own operations in the kernel's order (this file is compiled -ffp-contract=off like the kernels).
void fill_bil1(float *h, int size, float sigma_spatial, float sigma_color)
{
    const int D = size >> 12, zd = size & 4095;
    std::vector<float> g2(15 * 15), g1((size_t)(D > 0 ? D : 1));
    gaussian_kernel_2d(g2.data(), 7, sigma_spatial);
    gaussian_kernel_1d(g1.data(), D, sigma_color);
    const float gc = g1[0];
    for (int i = 0; i < D; ++i) {
        const float c = (float)(i - zd);
        volatile float norm = 0.0f, res = 0.0f;
        for (int t = 0; t < 15 * 15; ++t) {
            volatile float w = g2[t] * gc;
            norm = norm + w;
            volatile float cw = c * w;
            res = res + cw;
        }
        h[i] = res / norm;
    }
}
const float *bilateral_one_value_table(int D, int zd, float sigma_spatial, float sigma_color)
{
    if (D < 1 || D >= (1 << 19) || zd < 0 || zd >= 4096) return nullptr;
    return dev_table(3, D * 4096 + zd, sigma_spatial, sigma_color, (size_t)D, fill_bil1);
}

void sync() { STM_CHECK(hipStreamSynchronize(stream())); }

template <class T> T *up(const T *h, size_t n)
{
    T *d = Workspace::get<T>(n);
    STM_CHECK(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, stream()));
    return d;
}
template <class T> void down(T *h, const T *d, size_t n)
{
    STM_CHECK(hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, stream()));
}
float *up_planes(float **planes, int D, size_t HW)
{
    float *slab = Workspace::get<float>((size_t)D * HW);
    for (int d = 0; d < D; ++d)
        STM_CHECK(hipMemcpyAsync(slab + (size_t)d * HW, planes[d], HW * sizeof(float), hipMemcpyHostToDevice, stream()));
    return slab;
}
void down_planes(float **planes, const float *slab, int D, size_t HW)
{
    for (int d = 0; d < D; ++d)
        STM_CHECK(hipMemcpyAsync(planes[d], slab + (size_t)d * HW, HW * sizeof(float), hipMemcpyDeviceToHost, stream()));
}
// the views of a host-flavour interlacer or quilt uploaded, and their device table
u8 **up_views(unsigned char **views, int num_views, size_t in_sz)
{
    std::vector<u8 *> h(num_views);
    for (int v = 0; v < num_views; ++v) h[v] = up(views[v], in_sz);
    u8 **dv = Workspace::get<u8 *>(num_views);
    STM_CHECK(hipMemcpyAsync(dv, h.data(), sizeof(u8 *) * num_views, hipMemcpyHostToDevice, stream()));
    sync(); // h goes out of scope here
    return dv;
}

struct Arms {
    u8 *up, *down, *left, *right;
};

// Argument screen shared by every entry point.  The reference checks nothing (a zero-sized launch or an
// out-of-range view index is undefined behaviour there); here such calls fail like any other error (stm_hip.h).
struct Dim { const char *name; int v, lo; };
bool args_ok(const char *fn, std::initializer_list<Dim> dims)
{
    if (api_outermost()) clear_failed(); // every entry point starts here: a failure is sticky for one (outermost) API call (stm_common.h)
    for (const Dim &d : dims)
        if (d.v < d.lo) return STM_REJECT(d.name, "%s: %s = %d, must be >= %d", fn, d.name, d.v, d.lo);
    return true;
}


// ---------------------------------------------------------------- device cores
// cost init: pack -> census -> fused AD + census + robust combine
// packed_ready: pk_l / pk_r already hold the BGRX dwords of the two images (launch_demux_sbs_packed)
// census_out != nullptr: stop after the census planes (returned there) -- the caller computes the costs on the fly
// census_ready: the two census planes, already filled together with the packed planes (launch_front)
void core_ci(const u8 *d_img_l, const u8 *d_img_r, Vol cl, Vol cr, uint32_t *pk_l, uint32_t *pk_r, float ad_coeff,
             float census_coeff, int D, int zd, int H, int W, int elem_sz, bool packed_ready = false,
             uint32_t **census_out = nullptr, uint32_t *const *census_ready = nullptr)
{
    size_t HW = (size_t)H * W;
    uint32_t *cen_l = census_ready ? census_ready[0] : Workspace::get<uint32_t>(HW), *cen_r = census_ready ? census_ready[1] : Workspace::get<uint32_t>(HW);
    if (!packed_ready) {
        launch_pack_bgrx(d_img_l, pk_l, H, W, elem_sz);
        launch_pack_bgrx(d_img_r, pk_r, H, W, elem_sz);
    }
    if (!census_ready) launch_census32_pair(pk_l, cen_l, pk_r, cen_r, H, W);
    if (census_out) {
        census_out[0] = cen_l;
        census_out[1] = cen_r;
        return;
    }
    const float *lut = rho_table(ad_coeff, census_coeff);
    launch_cost_init(pk_l, pk_r, cen_l, cen_r, cl, cr, lut, lut + 768, D, zd, H, W);
    if (ref_quirks()) launch_cost_quirks(pk_l, pk_r, cen_l, cen_r, cl, cr, lut, lut + 768, D, zd, H, W); // per-stage ci_adcensus only (stm_hip.h)
}

// aggregation H, V, V, H (d_ca_cross.cu:255-270 minus the transposes); result ends in `cost`
// scratch.base == nullptr: carved here when the vector-ALU kernels run (a plane slab of D * H * W floats)
static bool agg_on_matrix_pipe(int usd, int H, int W) { return (agg_variant() / 10000) % 10 != 1 && aggm_supports(usd, H, W); }
// the `stages` bits of a frame call that decide what its aggregation chain has to leave behind (frame_disparity's hslo and subpix)
static bool stages_hslo(int stages) { return (stages & 0x100) != 0; }   // + scanline optimisation between aggregation and WTA (BASELINE config 3)
static bool stages_subpix(int stages) { return (stages & 0x200) != 0; } // + sub-pixel enhancement of the whole-pixel maps (Mei et al. 3.4)
// stm_agg_path (stm_hip.h): the same predicates, in the same order, as frame_disparity and launch_aggm_frame
int frame_agg_path(int D, int zd, int H, int W, int usd, int stages)
{
    if (D < 1 || H < 1 || W < 1 || !agg_on_matrix_pipe(usd, H, W)) return 0;
    return 1 | aggm_frame_path(D, zd, H, W, usd, stages_hslo(stages), stages_subpix(stages));
}
// stm_first_pass_path (stm_hip.h): the same predicates again
int frame_first_pass_path(int D, int zd, int H, int W, int usd, int stages)
{
    if (D < 1 || H < 1 || W < 1 || !agg_on_matrix_pipe(usd, H, W)) return 0;
    return aggm_frame_hc2_parts(D, zd, H, W, usd, stages_hslo(stages), stages_subpix(stages));
}
// stm_px_order (stm_hip.h): the same predicates again
int frame_px_order(int D, int zd, int H, int W, int usd, int stages)
{
    if (D < 1 || H < 1 || W < 1 || !agg_on_matrix_pipe(usd, H, W)) return -1;
    return aggm_frame_px_order(D, zd, H, W, usd, stages_hslo(stages), stages_subpix(stages));
}
void core_agg(Vol cost, Vol scratch, const Arms &a, int D, int H, int W, int usd)
{
    // the frame pipeline's matrix-pipe kernels (round 3) -- unless the caller's volume holds infinities, NaNs or denormals
    if (agg_on_matrix_pipe(usd, H, W) && launch_aggm_stage(cost, cost, a.up, a.down, a.left, a.right, D, H, W, usd)) return;
    if (!scratch.base && !scratch.tab) scratch = vol_slab(Workspace::get<float>((size_t)D * H * W), (size_t)H * W);
    launch_agg_h(cost, scratch, a.left, a.right, D, H, W);
    launch_agg_v(scratch, cost, a.up, a.down, D, H, W, usd);
    launch_agg_v(cost, scratch, a.up, a.down, D, H, W, usd);
    launch_agg_h(scratch, cost, a.left, a.right, D, H, W);
}
Arms carve_arms(size_t HW)
{
    u8 *m = Workspace::get<u8>(4 * HW);
    return Arms{m, m + HW, m + 2 * HW, m + 3 * HW};
}
Arms arms_from_table(unsigned char **d_cross)
{
    // the reference hands the four plane pointers over as a DEVICE table (d_io.cu:94-101); fetch them
    u8 *h[4];
    STM_CHECK(hipMemcpyAsync(h, d_cross, sizeof h, hipMemcpyDeviceToHost, stream()));
    sync();
    return Arms{h[0], h[1], h[2], h[3]};
}

void core_bilateral(float *d_img, int radius, float sigma_color, float sigma_spatial, int H, int W, int D)
{
    size_t HW = (size_t)H * W;
    float *tmp = Workspace::get<float>(HW);
    launch_bilateral(d_img, tmp, gauss2d_table(radius, sigma_spatial), gauss1d_table(D, sigma_color), radius, H, W, D);
    STM_CHECK(hipMemcpyAsync(d_img, tmp, HW * sizeof(float), hipMemcpyDeviceToDevice, stream())); // d_filter_bilateral.cu:560
}

void core_dbm(u8 *d_out, const u8 *d_l, const u8 *d_r, const float *disp_l, const float *disp_r, const float *mask_l,
              const float *mask_r, float shift, int H, int W, int elem_sz, int g_radius, float g_sigma, bool linear = false)
{
    size_t HW = (size_t)H * W;
    float *blend = Workspace::get<float>(HW);
    launch_gaussian_max(mask_r, blend, gauss2d_table(g_radius, g_sigma), g_radius, g_sigma, H, W, true); // G(1 - maskR)
    launch_view_synth(d_out, d_l, d_r, disp_l, disp_r, mask_l, mask_r, blend, shift, H, W, elem_sz, linear);
}

// dibr_dbm / dibr_dbm_lin: one body per flavour, `linear` selects the fetch of the two backward warps (stm_hip.h)
void dbm_device(const char *fn, unsigned char *d_img_out, unsigned char *d_img_in_l, unsigned char *d_img_in_r, float *d_disp_l,
                float *d_disp_r, float *d_mask_l, float *d_mask_r, float shift, int num_rows, int num_cols, int elem_sz, bool linear)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}})) return;
    Workspace::begin((size_t)num_rows * num_cols * 4 + 1024);
    if (elem_sz > 3) // d_dibr_bwarp.cu:53: the bytes of a pixel past the third come out 0 (the kernel writes the first three of every pixel)
        STM_CHECK(hipMemsetAsync(d_img_out, 0, (size_t)num_rows * num_cols * elem_sz, stream()));
    core_dbm(d_img_out, d_img_in_l, d_img_in_r, d_disp_l, d_disp_r, d_mask_l, d_mask_r, shift, num_rows, num_cols, elem_sz,
             10, 15.0f, linear); // d_dibr_bwarp.cu:63
}
void dbm_host(const char *fn, unsigned char *img_out, unsigned char *img_in_l, unsigned char *img_in_r, float *disp_l, float *disp_r,
              float *mask_l, float *mask_r, float shift, int num_rows, int num_cols, int elem_sz, bool linear)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(3 * HW * elem_sz + 20 * HW + 8192);
    u8 *l = up(img_in_l, HW * elem_sz), *r = up(img_in_r, HW * elem_sz), *o = Workspace::get<u8>(HW * elem_sz);
    float *dl = up(disp_l, HW), *dr = up(disp_r, HW), *ml = up(mask_l, HW), *mr = up(mask_r, HW);
    STM_CHECK(hipMemsetAsync(o, 0, HW * elem_sz, stream())); // d_dibr_bwarp.cu:136: bytes past a pixel's third come back 0, not as the workspace held them
    core_dbm(o, l, r, dl, dr, ml, mr, shift, num_rows, num_cols, elem_sz, 7, 10.0f, linear); // d_dibr_bwarp.cu:151
    down(img_out, o, HW * elem_sz);
    sync();
}

// the reference's view assignment from `angle`: y_interval, 1 / y_interval and round(y_interval) (any of the three may be null);
// false with the error recorded
bool mux_geom_ok(int N, float angle, int elem_sz, float *y_interval, float *inv_y_interval, int *ymod_out)
{
    float yi = mux_y_interval(N, angle, elem_sz);
    // tan(angle) = 0 divides by zero in the reference (d_mux_multiview.cu:146, SURVEY A-Q24); a period beyond the int
    // range would make the (int) conversion undefined
    if (!(fabsf(yi) < 1.0e9f)) return STM_REJECT("angle", "mux_multiview: y_interval is not finite (tan(angle) == 0 or angle is not a number)");
    int ymod = (int)roundf(yi);
    if (ymod == 0) return STM_REJECT("ymod", "mux_multiview: round(y_interval) == 0 (angle too steep)");
    if (y_interval) *y_interval = yi;
    if (inv_y_interval) *inv_y_interval = 1.0f / yi;
    if (ymod_out) *ymod_out = ymod;
    return true;
}
void core_mux(const u8 *const *d_views, u8 *d_out, int N, float angle, int Hin, int Win, int Hout, int Wout, int elem_sz,
              int variant)
{
    float yi, inv_y;
    int ymod;
    if (!mux_geom_ok(N, angle, elem_sz, &yi, &inv_y, &ymod)) return;
    launch_mux(d_views, d_out, N, yi, inv_y, ymod, Hin, Win, Hout, Wout, elem_sz, variant);
}
// a quilt's tiles go along the compositor's third grid dimension
bool overlay_tiles_ok(const char *fn, const Layout &lo, int num_views)
{
    if (lo.layout == 0 || num_views <= 65535) return true;
    return STM_REJECT("num_views", "%s: an overlay on a quilt of %d tiles: at most 65535 tiles", fn, num_views);
}

// guided up-sampling: the dimension screen, then sigma_color (stm_hip.h)
bool upsample_args_ok(const char *fn, int out_rows, int out_cols, int in_rows, int in_cols, int elem_sz, float sigma_color)
{
    if (!args_ok(fn, {{"out_rows", out_rows, 1}, {"out_cols", out_cols, 1}, {"in_rows", in_rows, 1}, {"in_cols", in_cols, 1},
                      {"elem_sz", elem_sz, 3}}))
        return false;
    if (!(sigma_color > 0.0f)) // 0, negative, NaN: the table would hold 0 / 0
        return STM_REJECT("sigma_color", "%s: sigma_color = %g, must be > 0", fn, (double)sigma_color);
    return true;
}
// the three parameters of the temporal stabilisation (stm_hip.h): 0 <= alpha <= 1, 0 <= thresh_color <= 765, thresh_disp >= 0
// (+inf allowed); a NaN fails every one of these comparisons
bool temporal_params_ok(const char *fn, float alpha, int thresh_color, float thresh_disp)
{
    if (!(alpha >= 0.0f && alpha <= 1.0f)) return STM_REJECT("alpha", "%s: alpha = %g, must be in [0, 1]", fn, (double)alpha);
    if (thresh_color < 0 || thresh_color > 765) return STM_REJECT("thresh_color", "%s: thresh_color = %d, must be in [0, 765]", fn, thresh_color);
    if (!(thresh_disp >= 0.0f)) return STM_REJECT("thresh_disp", "%s: thresh_disp = %g, must be >= 0", fn, (double)thresh_disp);
    return true;
}
// two maps of n floats each share at least one element
bool maps_overlap(const float *a, const float *b, size_t n)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b, bytes = n * sizeof(float);
    return pa < pb + bytes && pb < pa + bytes;
}
bool temporal_args_ok(const char *fn, const float *disp, const float *disp_prev, int num_rows, int num_cols, int elem_sz, float alpha,
                      int thresh_color, float thresh_disp)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}})) return false;
    if (!temporal_params_ok(fn, alpha, thresh_color, thresh_disp)) return false;
    if (disp && disp_prev && maps_overlap(disp, disp_prev, (size_t)num_rows * num_cols)) // the map is rewritten in place
        return STM_REJECT("disp_prev", "%s: disp_prev must not alias disp", fn);
    return true;
}
// [a, a + n) and [b, b + m) share a byte
bool bytes_overlap(const void *a, size_t n, const void *b, size_t m)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + m && pb < pa + n;
}
} // namespace

// the overlay composited on the finished frame d_frame, rendered under ln and lo (stm_common.h).  In lens mode 0 of layout 0 the
// sub-pixels' views follow from `angle` as in the frame's interlacer, whose screen the frame call has already passed
void stm::frame_overlay(u8 *d_frame, const Overlay &ov, const Lens &ln, const Layout &lo, int num_views, float angle, int Hout, int Wout,
                        int elem_sz)
{
    float yi = 0.0f, inv_y = 0.0f;
    int ymod = 1;
    if (lo.layout == 0 && ln.mode == 0 && !mux_geom_ok(num_views, angle, elem_sz, &yi, &inv_y, &ymod)) return;
    launch_overlay(d_frame, ov.d_overlay, ov.ov_rows, ov.ov_cols, ov.x0, ov.y0, ov.disparity, num_views, ln, yi, inv_y, ymod, lo, Hout, Wout,
                   elem_sz, ov.d_disp, ov.limit_lo, ov.limit_hi);
}

// the overlay's fit on the maps the renderer read (stm_set_overlay_auto), then the overlay composited at the state's disparity: the
// setter's own disparity is ignored.  The view is the output frame in layout 0 and one tile of a quilt; the budget is (1, 0) in depth
// mode 0, the setting in mode 1 and depth_state's in mode 2.  The geometry is screened first: a frame the compositor would refuse is
// not measured either
void stm::frame_overlay_auto(u8 *d_frame, const Overlay &ov, const OverlayAuto &oa, float *state, uint32_t *ws, bool fresh, bool zero_state, const float *d_disp_l,
                             const float *d_disp_r, int H, int W, const Depth &dp, const float *depth_state, const int *cut_state, const Lens &ln,
                             const Layout &lo, int num_views, float angle, int Hout, int Wout, int elem_sz, const int *d_rect)
{
    if (lo.layout == 0 && ln.mode == 0 && !mux_geom_ok(num_views, angle, elem_sz, nullptr, nullptr, nullptr)) return;
    const int Hv = lo.layout == 1 ? Hout / lo.tiles_y : Hout, Wv = lo.layout == 1 ? Wout / lo.tiles_x : Wout;
    launch_overlay_fit(state, ws, d_disp_l, d_disp_r, H, W, ov.d_overlay, ov.ov_rows, ov.ov_cols, ov.x0, ov.y0, Hv, Wv, dp.mode == 1 ? dp.gain : 1.0f,
                       dp.mode == 1 ? dp.conv : 0.0f, dp.mode == 2 ? depth_state : nullptr, oa, fresh, zero_state, cut_state, d_rect);
    Overlay at = ov;
    at.d_disp = state + 1;
    at.limit_lo = oa.limit_lo;
    at.limit_hi = oa.limit_hi;
    frame_overlay(d_frame, at, ln, lo, num_views, angle, Hout, Wout, elem_sz);
}

// the two pitches and the matrix of NV12 planes num_cols_sbs samples wide: the tail of the plain and of the packed frame's rules
static bool nv12_planes_ok(const char *fn, int num_cols_sbs, int pitch_y, int pitch_uv, int matrix)
{
    if (pitch_y < num_cols_sbs) return STM_REJECT("pitch_y", "%s: pitch_y = %d, must be >= num_cols_sbs = %d", fn, pitch_y, num_cols_sbs);
    if (pitch_uv < 2 * ((num_cols_sbs + 1) / 2))
        return STM_REJECT("pitch_uv", "%s: pitch_uv = %d, must be >= 2 * ((num_cols_sbs + 1) / 2) = %d", fn, pitch_uv, 2 * ((num_cols_sbs + 1) / 2));
    if (matrix < 0 || matrix > 3)
        return STM_REJECT("matrix", "%s: matrix = %d, must be 0 (BT.601 limited), 1 (BT.709 limited), 2 (BT.601 full) or 3 (BT.709 full)", fn, matrix);
    return true;
}
// the rules of an NV12 frame (stm_hip.h, stm_demux_nv12), after the dimension screen; cols_name: what the call names the width of a view
bool stm::nv12_args_ok(const char *fn, int num_rows, int num_cols_sbs, int num_cols, const char *cols_name, int pitch_y, int pitch_uv,
                       int matrix)
{
    if (num_rows & 1) return STM_REJECT("num_rows", "%s: num_rows = %d, must be even (a chroma row serves two rows)", fn, num_rows);
    if (num_cols & 1) return STM_REJECT(cols_name, "%s: %s = %d, must be even (each half starts on a chroma sample)", fn, cols_name, num_cols);
    if (num_cols_sbs < 2 * num_cols)
        return STM_REJECT("num_cols_sbs", "%s: num_cols_sbs = %d, must be >= 2 * %s = %d", fn, num_cols_sbs, cols_name, 2 * num_cols);
    return nv12_planes_ok(fn, num_cols_sbs, pitch_y, pitch_uv, matrix);
}

// the rules of a packed frame (stm_hip.h, stm_demux_packed), after the dimension screen
bool stm::quilt_args_ok(const char *fn, const Layout &lo, int num_views, int in_rows, int in_cols, int out_rows, int out_cols,
                        const char *views_name, const char *rows_name, const char *cols_name)
{
    const int tw = out_cols / lo.tiles_x, th = out_rows / lo.tiles_y;
    if ((long long)lo.tiles_x * lo.tiles_y != num_views)
        return STM_REJECT(views_name, "%s: a quilt of tiles_x * tiles_y = %d * %d tiles needs as many views, %s = %d", fn, lo.tiles_x, lo.tiles_y,
                          views_name, num_views);
    if (tw == 0) return STM_REJECT(cols_name, "%s: %s = %d leaves tiles_x = %d tiles no column", fn, cols_name, out_cols, lo.tiles_x);
    if (th == 0) return STM_REJECT(rows_name, "%s: %s = %d leaves tiles_y = %d tiles no row", fn, rows_name, out_rows, lo.tiles_y);
    if ((long long)tw * in_cols > 0x7fffffffll) // the area filter's weights are ints
        return STM_REJECT(cols_name, "%s: tile width * view width = %d * %d does not fit 31 bits (%s)", fn, tw, in_cols, cols_name);
    if ((long long)th * in_rows > 0x7fffffffll)
        return STM_REJECT(rows_name, "%s: tile height * view height = %d * %d does not fit 31 bits (%s)", fn, th, in_rows, rows_name);
    return true;
}
bool stm::packing_args_ok(const char *fn, const Packing &pk, int num_rows, int num_cols_sbs, int num_cols, const char *cols_name, bool nv12,
                          int pitch_y, int pitch_uv, int matrix)
{
    if (!packing_params_ok(fn, pk)) return false;
    const int H = num_rows, W = num_cols, half = pk.packing & 1, axis = pk.packing >> 1;
    const long long need = axis == 0 ? 2LL * (half ? W / 2 : W) + pk.gap : W; // the row the rule asks for
    if (pk.packing == 1 && (W & 1))
        return STM_REJECT(cols_name, "%s: %s = %d, must be even with packing 1 (each eye is squeezed to half the columns)", fn, cols_name, W);
    if (pk.packing == 3 && (H & 1))
        return STM_REJECT("num_rows", "%s: num_rows = %d, must be even with packing 3 (each eye is squeezed to half the rows)", fn, H);
    if (num_cols_sbs < need)
        return STM_REJECT("num_cols_sbs", "%s: num_cols_sbs = %d, must be >= %lld with packing %d, gap %d and %s = %d", fn, num_cols_sbs, need,
                          pk.packing, pk.gap, cols_name, W);
    if (!nv12) return true;
    if ((H & 1) || (pk.packing == 3 && (H & 3)))
        return STM_REJECT("num_rows", "%s: num_rows = %d, must be a multiple of %d for NV12 with packing %d (each packed eye has an even number of rows)",
                          fn, H, pk.packing == 3 ? 4 : 2, pk.packing);
    if ((W & 1) || (pk.packing == 1 && (W & 3)))
        return STM_REJECT(cols_name, "%s: %s = %d, must be a multiple of %d for NV12 with packing %d (each packed eye starts on a chroma sample)",
                          fn, cols_name, W, pk.packing == 1 ? 4 : 2, pk.packing);
    if (pk.gap & 1) return STM_REJECT("gap", "%s: gap = %d, must be even for NV12 (the second eye starts on a chroma sample)", fn, pk.gap);
    return nv12_planes_ok(fn, num_cols_sbs, pitch_y, pitch_uv, matrix);
}

extern "C" {

// =============================================================== cost init
void stm_d_ci_adcensus(unsigned char *d_img_l, unsigned char *d_img_r, float **d_adcensus_cost_l,
                       float **d_adcensus_cost_r, float **h_adcensus_cost_l, float **h_adcensus_cost_r,
                       float *d_adcensus_cost_memory, float ad_coeff, float census_coeff, int num_disp, int zero_disp,
                       int num_rows, int num_cols, int elem_sz)
{
    if (!args_ok("d_ci_adcensus", {{"num_disp", num_disp, 1}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1},
                                   {"elem_sz", elem_sz, 3}}))
        return;
    size_t HW = (size_t)num_rows * num_cols, V = HW * num_disp;
    Workspace::begin(4 * HW * 4 + 4096);
    for (int d = 0; d < num_disp; ++d) { // d_ci_adcensus.cu:150-157
        h_adcensus_cost_l[d] = d_adcensus_cost_memory + (size_t)d * HW;
        h_adcensus_cost_r[d] = d_adcensus_cost_memory + (size_t)d * HW + V;
    }
    STM_CHECK(hipMemcpyAsync(d_adcensus_cost_l, h_adcensus_cost_l, sizeof(float *) * num_disp, hipMemcpyHostToDevice, stream()));
    STM_CHECK(hipMemcpyAsync(d_adcensus_cost_r, h_adcensus_cost_r, sizeof(float *) * num_disp, hipMemcpyHostToDevice, stream()));
    uint32_t *pk_l = Workspace::get<uint32_t>(HW), *pk_r = Workspace::get<uint32_t>(HW);
    core_ci(d_img_l, d_img_r, vol_slab(d_adcensus_cost_memory, HW), vol_slab(d_adcensus_cost_memory + V, HW), pk_l, pk_r,
            ad_coeff, census_coeff, num_disp, zero_disp, num_rows, num_cols, elem_sz);
}

void stm_ci_adcensus(unsigned char *img_l, unsigned char *img_r, float **cost_l, float **cost_r, float ad_coeff,
                     float census_coeff, int num_disp, int zero_disp, int num_rows, int num_cols, int elem_sz)
{
    if (!args_ok("ci_adcensus", {{"num_disp", num_disp, 1}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1},
                                 {"elem_sz", elem_sz, 3}}))
        return;
    size_t HW = (size_t)num_rows * num_cols, V = HW * num_disp;
    Workspace::begin(2 * V * 4 + 2 * HW * elem_sz + 4 * HW * 4 + 8192);
    u8 *dl = up(img_l, HW * elem_sz), *dr = up(img_r, HW * elem_sz);
    float *slab = Workspace::get<float>(2 * V);
    uint32_t *pk_l = Workspace::get<uint32_t>(HW), *pk_r = Workspace::get<uint32_t>(HW);
    core_ci(dl, dr, vol_slab(slab, HW), vol_slab(slab + V, HW), pk_l, pk_r, ad_coeff, census_coeff, num_disp, zero_disp,
            num_rows, num_cols, elem_sz);
    down_planes(cost_l, slab, num_disp, HW);
    down_planes(cost_r, slab + V, num_disp, HW);
    sync();
}

// =============================================================== aggregation
void stm_d_ca_cross(unsigned char *d_img, float **d_cost, float **d_acost, float **h_acost, float *d_acost_memory,
                    unsigned char **d_cross, float ucd, float lcd, int usd, int lsd, int num_disp, int num_rows,
                    int num_cols, int elem_sz)
{
    if (!args_ok("d_ca_cross", {{"num_disp", num_disp, 1}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1},
                                {"elem_sz", elem_sz, 3}}))
        return;
    size_t HW = (size_t)num_rows * num_cols;
    // (what launch_aggm_stage carves is part of the hint: no allocation happens inside the call once the slab has this size)
    Workspace::begin(12 * HW + 8192 + (agg_on_matrix_pipe(usd, num_rows, num_cols) ? aggm_stage_bytes(num_disp, num_rows, num_cols, usd) : 0));
    for (int d = 0; d < num_disp; ++d) h_acost[d] = d_acost_memory + (size_t)d * HW; // d_ca_cross.cu:207-210
    STM_CHECK(hipMemcpyAsync(d_acost, h_acost, sizeof(float *) * num_disp, hipMemcpyHostToDevice, stream()));
    Arms a = arms_from_table(d_cross);
    uint32_t *pk = Workspace::get<uint32_t>(HW);
    launch_pack_bgrx(d_img, pk, num_rows, num_cols, elem_sz);
    launch_cross_arms(pk, a.up, a.down, a.left, a.right, ucd, lcd, usd, lsd, num_rows, num_cols);
    core_agg(vol_table(d_cost), vol_slab(d_acost_memory, HW), a, num_disp, num_rows, num_cols, usd); // result in d_cost (A-Q11)
}

void stm_ca_cross(unsigned char *img, unsigned char **cross, float **cost, float **acost, float ucd, float lcd, int usd,
                  int lsd, int num_disp, int num_rows, int num_cols, int elem_sz)
{
    if (!args_ok("ca_cross", {{"num_disp", num_disp, 1}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1},
                              {"elem_sz", elem_sz, 3}}))
        return;
    size_t HW = (size_t)num_rows * num_cols, V = HW * num_disp;
    const bool mp = agg_on_matrix_pipe(usd, num_rows, num_cols);
    Workspace::begin(V * 4 + HW * elem_sz + 12 * HW + 16384 + (mp ? aggm_stage_bytes(num_disp, num_rows, num_cols, usd) : V * 4));
    u8 *dimg = up(img, HW * elem_sz);
    float *c = up_planes(cost, num_disp, HW);
    float *s = mp ? nullptr : Workspace::get<float>(V); // the vector-ALU kernels' scratch volume (carved late if they run as the fallback)
    Arms a = carve_arms(HW);
    uint32_t *pk = Workspace::get<uint32_t>(HW);
    launch_pack_bgrx(dimg, pk, num_rows, num_cols, elem_sz);
    launch_cross_arms(pk, a.up, a.down, a.left, a.right, ucd, lcd, usd, lsd, num_rows, num_cols);
    core_agg(vol_slab(c, HW), vol_slab(s, HW), a, num_disp, num_rows, num_cols, usd);
    down_planes(acost, c, num_disp, HW); // d_ca_cross.cu:419-422: the "cost" device buffer goes to acost
    down(cross[0], a.up, HW); down(cross[1], a.down, HW); down(cross[2], a.left, HW); down(cross[3], a.right, HW);
    sync();
}

// =============================================================== disparity selection
void stm_d_dc_wta(float **d_cost, float *d_disp, int num_disp, int zero_disp, int num_rows, int num_cols)
{
    if (!args_ok("d_dc_wta", {{"num_disp", num_disp, 1}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    launch_wta(vol_table(d_cost), d_disp, num_disp, zero_disp, num_rows, num_cols);
}
void stm_dc_wta(float **cost, float *disp, int num_disp, int zero_disp, int num_rows, int num_cols)
{
    if (!args_ok("dc_wta", {{"num_disp", num_disp, 1}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin((size_t)num_disp * HW * 4 + HW * 4 + 4096);
    float *c = up_planes(cost, num_disp, HW);
    float *d = Workspace::get<float>(HW);
    launch_wta(vol_slab(c, HW), d, num_disp, zero_disp, num_rows, num_cols);
    down(disp, d, HW);
    sync();
}

// sub-pixel enhancement (Mei et al. 3.4; an addition, the reference has none): disp refined in place, cost as for dc_wta
void stm_d_dc_subpixel(float **d_cost, float *d_disp, int num_disp, int zero_disp, int num_rows, int num_cols)
{
    if (!args_ok("d_dc_subpixel", {{"num_disp", num_disp, 1}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    launch_subpix(vol_table(d_cost), d_disp, num_disp, zero_disp, num_rows, num_cols);
}
void stm_dc_subpixel(float **cost, float *disp, int num_disp, int zero_disp, int num_rows, int num_cols)
{
    if (!args_ok("dc_subpixel", {{"num_disp", num_disp, 1}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin((size_t)num_disp * HW * 4 + HW * 4 + 4096);
    float *c = up_planes(cost, num_disp, HW);
    float *d = up(disp, HW);
    launch_subpix(vol_slab(c, HW), d, num_disp, zero_disp, num_rows, num_cols);
    down(disp, d, HW);
    sync();
}

// d_dc_hslo and d_dc_hslo_view (include/stm_hslo_tap.h) behind their screens: one view's volume, the view's own image and the other one,
// osign = +1 (left view) / -1 (right view)
static void d_dc_hslo_rect(float **d_cost, float *d_disp, unsigned char *d_img_own, unsigned char *d_img_other, float T, float H1,
                           float H2, int num_disp, int zero_disp, int num_rows, int num_cols, int elem_sz, int osign)
{
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin((size_t)((num_disp + 3) / 4) * HW * 16 * 6 + 16 * HW + 16384);
    Vol c = vol_table(d_cost);
    const u8 *ia[1] = {d_img_own}, *ib[1] = {d_img_other};
    const int os[1] = {osign};
    float *dv[1] = {d_disp};
    launch_hslo_wta(1, &c, ia, ib, os, dv, T, H1, H2, num_disp, zero_disp, num_rows, num_cols, elem_sz);
}
void stm_d_dc_hslo(float **d_cost, float *d_disp, unsigned char *d_img_l, unsigned char *d_img_r, float T, float H1,
                   float H2, int num_disp, int zero_disp, int num_rows, int num_cols, int elem_sz)
{
    if (!args_ok("d_dc_hslo", {{"num_disp", num_disp, 1}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1},
                               {"elem_sz", elem_sz, 3}}))
        return;
    d_dc_hslo_rect(d_cost, d_disp, d_img_l, d_img_r, T, H1, H2, num_disp, zero_disp, num_rows, num_cols, elem_sz, 1);
}
static bool hslo_view_ok(const char *fn, int view)
{
    if (view < 0 || view > 1) return STM_REJECT("view", "%s: view = %d, must be 0 (the left view) or 1 (the right view)", fn, view);
    return true;
}
void stm_d_dc_hslo_view(float **d_cost, float *d_disp, unsigned char *d_img_own, unsigned char *d_img_other, float T, float H1,
                        float H2, int num_disp, int zero_disp, int num_rows, int num_cols, int elem_sz, int view)
{
    if (!args_ok("d_dc_hslo_view", {{"num_disp", num_disp, 1}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1},
                                    {"elem_sz", elem_sz, 3}}) ||
        !hslo_view_ok("d_dc_hslo_view", view))
        return;
    d_dc_hslo_rect(d_cost, d_disp, d_img_own, d_img_other, T, H1, H2, num_disp, zero_disp, num_rows, num_cols, elem_sz, view ? -1 : 1);
}
int stm_set_hslo_tap(float *d_s2, float *d_s3, float *d_fin)
{
    if (api_outermost()) clear_failed();
    const void *p[3] = {d_s2, d_s3, d_fin};
    const char *name[3] = {"d_s2", "d_s3", "d_fin"};
    for (int i = 0; i < 3; ++i)
        if (((uintptr_t)p[i] & 3) != 0) // the thread's tap stays as it was
            return STM_REJECT(name[i], "set_hslo_tap: %s must be 4-byte aligned (a volume of floats)", name[i]) ? 0 : -1;
    set_hslo_tap(HsloTap{d_s2, d_s3, d_fin});
    return 0;
}
void stm_dc_hslo(float **cost, float *disp, unsigned char *img_l, unsigned char *img_r, float T, float H1, float H2,
                 int num_disp, int zero_disp, int num_rows, int num_cols, int elem_sz)
{
    if (!args_ok("dc_hslo", {{"num_disp", num_disp, 1}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1},
                             {"elem_sz", elem_sz, 3}}))
        return;
    size_t HW = (size_t)num_rows * num_cols, V = HW * num_disp;
    Workspace::begin(V * 4 + (size_t)((num_disp + 3) / 4) * HW * 16 * 6 + 2 * HW * elem_sz + 5 * HW * 4 + 32768);
    float *c = up_planes(cost, num_disp, HW);
    u8 *dl = up(img_l, HW * elem_sz), *dr = up(img_r, HW * elem_sz);
    float *d = Workspace::get<float>(HW);
    Vol cv = vol_slab(c, HW);
    const u8 *ia[1] = {dl}, *ib[1] = {dr};
    const int os[1] = {1};
    float *dv[1] = {d};
    launch_hslo_wta(1, &cv, ia, ib, os, dv, T, H1, H2, num_disp, zero_disp, num_rows, num_cols, elem_sz);
    down(disp, d, HW);
    sync();
}

// =============================================================== refinement
void stm_d_dr_dcc(unsigned char *d_outliers_l, unsigned char *d_outliers_r, float *d_disp_l, float *d_disp_r, int num_rows,
                  int num_cols)
{
    if (!args_ok("d_dr_dcc", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(2 * HW + 1024);
    u8 *hl = Workspace::get<u8>(HW), *hr = Workspace::get<u8>(HW);
    launch_dcc(d_outliers_l, d_outliers_r, d_disp_l, d_disp_r, hl, hr, num_rows, num_cols);
}
void stm_dr_dcc(unsigned char *outliers_l, unsigned char *outliers_r, float *disp_l, float *disp_r, int num_rows,
                int num_cols)
{
    if (!args_ok("dr_dcc", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(12 * HW + 4096);
    float *dl = up(disp_l, HW), *dr = up(disp_r, HW);
    u8 *ol = Workspace::get<u8>(HW), *orr = Workspace::get<u8>(HW), *hl = Workspace::get<u8>(HW), *hr = Workspace::get<u8>(HW);
    STM_CHECK(hipMemsetAsync(ol, 0, HW, stream())); // d_dr_dcc.cu:166-171
    STM_CHECK(hipMemsetAsync(orr, 0, HW, stream()));
    launch_dcc(ol, orr, dl, dr, hl, hr, num_rows, num_cols);
    down(outliers_l, ol, HW); down(outliers_r, orr, HW);
    sync();
}

void stm_d_dr_irv(float *d_disp, unsigned char *d_outliers, unsigned char **d_cross, int thresh_s, float thresh_h,
                  int num_rows, int num_cols, int num_disp, int zero_disp, int usd, int iterations)
{
    if (!args_ok("d_dr_irv", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"num_disp", num_disp, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(30 * HW + 65536);
    Arms a = arms_from_table(d_cross);
    float *dv[1] = {d_disp};
    u8 *ov[1] = {d_outliers};
    const u8 *u[1] = {a.up}, *d[1] = {a.down}, *l[1] = {a.left}, *r[1] = {a.right};
    launch_irv(1, dv, ov, u, d, l, r, thresh_s, thresh_h, num_rows, num_cols, num_disp, zero_disp, usd, iterations, true);
}
void stm_dr_irv(float *disp, unsigned char *outliers, unsigned char **cross, int thresh_s, float thresh_h, int num_rows,
                int num_cols, int num_disp, int zero_disp, int usd, int iterations)
{
    if (!args_ok("dr_irv", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"num_disp", num_disp, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(40 * HW + 65536);
    float *d = up(disp, HW);
    u8 *o = up(outliers, HW);
    Arms a{up(cross[0], HW), up(cross[1], HW), up(cross[2], HW), up(cross[3], HW)};
    float *dv[1] = {d};
    u8 *ov[1] = {o};
    const u8 *uu[1] = {a.up}, *dd[1] = {a.down}, *ll[1] = {a.left}, *rr[1] = {a.right};
    launch_irv(1, dv, ov, uu, dd, ll, rr, thresh_s, thresh_h, num_rows, num_cols, num_disp, zero_disp, usd, iterations, false);
    down(disp, d, HW); down(outliers, o, HW);
    sync();
}

// outlier interpolation (Mei et al. 3.4; an addition, the reference has none): disp refined in place where outliers != 0
void stm_d_dr_interp(float *d_disp, unsigned char *d_outliers, unsigned char *d_img, int num_rows, int num_cols, int elem_sz)
{
    if (!args_ok("d_dr_interp", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}})) return;
    float *dv[1] = {d_disp};
    const u8 *ov[1] = {d_outliers}, *iv[1] = {d_img};
    launch_interp(1, dv, ov, iv, num_rows, num_cols, elem_sz);
}
void stm_dr_interp(float *disp, unsigned char *outliers, unsigned char *img, int num_rows, int num_cols, int elem_sz)
{
    if (!args_ok("dr_interp", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin((5 + (size_t)elem_sz) * HW + 4096);
    float *d = up(disp, HW);
    u8 *o = up(outliers, HW), *im = up(img, HW * elem_sz);
    float *dv[1] = {d};
    const u8 *ov[1] = {o}, *iv[1] = {im};
    launch_interp(1, dv, ov, iv, num_rows, num_cols, elem_sz);
    down(disp, d, HW);
    sync();
}

void stm_d_filter_bilateral_1(float *d_img, int radius, float sigma_color, float sigma_spatial, int num_rows, int num_cols,
                              int num_disp)
{
    if (!args_ok("d_filter_bilateral_1", {{"radius", radius, 0}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1},
                                          {"num_disp", num_disp, 1}}))
        return;
    Workspace::begin((size_t)num_rows * num_cols * 4 + 1024);
    core_bilateral(d_img, radius, sigma_color, sigma_spatial, num_rows, num_cols, num_disp);
}
void stm_filter_bilateral_1(float *img, int radius, float sigma_color, float sigma_spatial, int num_rows, int num_cols,
                            int num_disp)
{
    if (!args_ok("filter_bilateral_1", {{"radius", radius, 0}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1},
                                        {"num_disp", num_disp, 1}}))
        return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(8 * HW + 4096);
    float *d = up(img, HW);
    core_bilateral(d, radius, sigma_color, sigma_spatial, num_rows, num_cols, num_disp);
    down(img, d, HW);
    sync();
}

void stm_d_filter_gaussian_1(float *d_img, int radius, float sigma_spatial, int num_rows, int num_cols)
{
    if (!args_ok("d_filter_gaussian_1", {{"radius", radius, 0}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(HW * 4 + 1024);
    float *tmp = Workspace::get<float>(HW);
    launch_gaussian_max(d_img, tmp, gauss2d_table(radius, sigma_spatial), radius, sigma_spatial, num_rows, num_cols, false);
    STM_CHECK(hipMemcpyAsync(d_img, tmp, HW * 4, hipMemcpyDeviceToDevice, stream())); // d_filter_gaussian.cu:171
}
void stm_filter_gaussian_1(float *img, int radius, float sigma_spatial, int num_rows, int num_cols)
{
    if (!args_ok("filter_gaussian_1", {{"radius", radius, 0}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(8 * HW + 4096);
    float *d = up(img, HW), *tmp = Workspace::get<float>(HW);
    launch_gaussian_max(d, tmp, gauss2d_table(radius, sigma_spatial), radius, sigma_spatial, num_rows, num_cols, false);
    down(img, tmp, HW);
    sync();
}

void stm_d_filter_bleed_1(unsigned char *d_img, int radius, int num_rows, int num_cols)
{
    if (!args_ok("d_filter_bleed_1", {{"radius", radius, 0}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(HW + 1024);
    u8 *tmp = Workspace::get<u8>(HW);
    launch_bleed(d_img, tmp, radius, num_rows, num_cols);
    STM_CHECK(hipMemcpyAsync(d_img, tmp, HW, hipMemcpyDeviceToDevice, stream())); // d_filter.cu:164
}
void stm_filter_bleed_1(unsigned char *img, int radius, int num_rows, int num_cols)
{
    if (!args_ok("filter_bleed_1", {{"radius", radius, 0}, {"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(2 * HW + 4096);
    u8 *d = up(img, HW), *tmp = Workspace::get<u8>(HW);
    launch_bleed(d, tmp, radius, num_rows, num_cols);
    down(img, tmp, HW);
    sync();
}

// d_filter.cu:47-103
void stm_d_filter_median(float *d_img, int num_rows, int num_cols)
{
    if (!args_ok("d_filter_median", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(HW * 4 + 1024);
    float *tmp = Workspace::get<float>(HW);
    launch_median3(d_img, tmp, num_rows, num_cols);
    STM_CHECK(hipMemcpyAsync(d_img, tmp, HW * 4, hipMemcpyDeviceToDevice, stream())); // d_filter.cu:67
}
void stm_filter_median(float *img, int num_rows, int num_cols)
{
    if (!args_ok("filter_median", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(8 * HW + 4096);
    float *d = up(img, HW), *tmp = Workspace::get<float>(HW);
    launch_median3(d, tmp, num_rows, num_cols);
    down(img, tmp, HW);
    sync();
}

// =============================================================== DIBR
void stm_d_dibr_occl(unsigned char *d_occl_l, unsigned char *d_occl_r, float *d_disp_l, float *d_disp_r, int num_rows,
                     int num_cols)
{
    if (!args_ok("d_dibr_occl", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    launch_occl(d_occl_l, d_occl_r, d_disp_l, d_disp_r, num_rows, num_cols);
}
void stm_dibr_occl(unsigned char *occl_l, unsigned char *occl_r, float *disp_l, float *disp_r, int num_rows, int num_cols)
{
    if (!args_ok("dibr_occl", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(10 * HW + 4096);
    float *dl = up(disp_l, HW), *dr = up(disp_r, HW);
    u8 *ol = Workspace::get<u8>(HW), *orr = Workspace::get<u8>(HW);
    launch_occl(ol, orr, dl, dr, num_rows, num_cols);
    down(occl_l, ol, HW); down(occl_r, orr, HW);
    sync();
}

void stm_d_dibr_occl_to_mask(float *d_mask_l, float *d_mask_r, unsigned char *d_occl_l, unsigned char *d_occl_r,
                             int num_rows, int num_cols)
{
    if (!args_ok("d_dibr_occl_to_mask", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    launch_occl_to_mask(d_mask_l, d_mask_r, d_occl_l, d_occl_r, num_rows, num_cols);
}
void stm_dibr_occl_to_mask(float *mask_l, float *mask_r, unsigned char *occl_l, unsigned char *occl_r, int num_rows,
                           int num_cols)
{
    if (!args_ok("dibr_occl_to_mask", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(10 * HW + 4096);
    u8 *ol = up(occl_l, HW), *orr = up(occl_r, HW);
    float *ml = Workspace::get<float>(HW), *mr = Workspace::get<float>(HW);
    launch_occl_to_mask(ml, mr, ol, orr, num_rows, num_cols);
    down(mask_l, ml, HW); down(mask_r, mr, HW);
    sync();
}

void stm_d_dibr_dbm(unsigned char *d_img_out, unsigned char *d_img_in_l, unsigned char *d_img_in_r, float *d_disp_l,
                    float *d_disp_r, unsigned char *d_occl_l, unsigned char *d_occl_r, float *d_mask_l, float *d_mask_r,
                    float shift, int num_rows, int num_cols, int elem_sz)
{
    (void)d_occl_l; (void)d_occl_r; // unused by the reference too (d_dibr_bwarp.cu:24-70)
    dbm_device("d_dibr_dbm", d_img_out, d_img_in_l, d_img_in_r, d_disp_l, d_disp_r, d_mask_l, d_mask_r, shift, num_rows, num_cols,
               elem_sz, false);
}
void stm_dibr_dbm(unsigned char *img_out, unsigned char *img_in_l, unsigned char *img_in_r, float *disp_l, float *disp_r,
                  unsigned char *occl_l, unsigned char *occl_r, float *mask_l, float *mask_r, float shift, int num_rows,
                  int num_cols, int elem_sz)
{
    (void)occl_l; (void)occl_r;
    dbm_host("dibr_dbm", img_out, img_in_l, img_in_r, disp_l, disp_r, mask_l, mask_r, shift, num_rows, num_cols, elem_sz, false);
}
// linear sampling (an addition, the reference has none): dibr_dbm with both backward warps fetched at the fractional coordinate
void stm_d_dibr_dbm_lin(unsigned char *d_img_out, unsigned char *d_img_in_l, unsigned char *d_img_in_r, float *d_disp_l,
                        float *d_disp_r, unsigned char *d_occl_l, unsigned char *d_occl_r, float *d_mask_l, float *d_mask_r,
                        float shift, int num_rows, int num_cols, int elem_sz)
{
    (void)d_occl_l; (void)d_occl_r;
    dbm_device("d_dibr_dbm_lin", d_img_out, d_img_in_l, d_img_in_r, d_disp_l, d_disp_r, d_mask_l, d_mask_r, shift, num_rows,
               num_cols, elem_sz, true);
}
void stm_dibr_dbm_lin(unsigned char *img_out, unsigned char *img_in_l, unsigned char *img_in_r, float *disp_l, float *disp_r,
                      unsigned char *occl_l, unsigned char *occl_r, float *mask_l, float *mask_r, float shift, int num_rows,
                      int num_cols, int elem_sz)
{
    (void)occl_l; (void)occl_r;
    dbm_host("dibr_dbm_lin", img_out, img_in_l, img_in_r, disp_l, disp_r, mask_l, mask_r, shift, num_rows, num_cols, elem_sz, true);
}

void stm_d_dibr_dfm(unsigned char *d_img_out, unsigned char *d_img_in_l, unsigned char *d_img_in_r, float *d_disp_l,
                    float *d_disp_r, float shift, int num_rows, int num_cols, int elem_sz)
{
    if (!args_ok("d_dibr_dfm", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}})) return;
    (void)d_img_in_r; (void)d_disp_r; // the right warp is computed and discarded in the reference (A-Q23)
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(HW * 8 + 1024);
    unsigned long long *keys = Workspace::get<unsigned long long>(HW);
    if (elem_sz > 3) // d_dibr_fwarp.cu:51,84: the whole cleared staging image is copied over d_img_out
        STM_CHECK(hipMemsetAsync(d_img_out, 0, HW * elem_sz, stream()));
    launch_fwarp(d_img_out, d_img_in_l, d_disp_l, shift, keys, num_rows, num_cols, elem_sz);
}
void stm_dibr_dfm(unsigned char *img_out, unsigned char *img_in_l, unsigned char *img_in_r, float *disp_l, float *disp_r,
                  float shift, int num_rows, int num_cols, int elem_sz)
{
    if (!args_ok("dibr_dfm", {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}})) return;
    (void)img_in_r; (void)disp_r;
    size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(2 * HW * elem_sz + 12 * HW + 8192);
    u8 *l = up(img_in_l, HW * elem_sz), *o = Workspace::get<u8>(HW * elem_sz);
    float *dl = up(disp_l, HW);
    unsigned long long *keys = Workspace::get<unsigned long long>(HW);
    STM_CHECK(hipMemsetAsync(o, 0, HW * elem_sz, stream())); // d_dibr_fwarp.cu:139
    launch_fwarp(o, l, dl, shift, keys, num_rows, num_cols, elem_sz);
    down(img_out, o, HW * elem_sz);
    sync();
}

// =============================================================== guided disparity up-sampling
// (an addition, the reference has none: its tx_disp_scale_kernel blends four low-resolution values whatever the image shows)
void stm_d_disp_upsample(float *d_disp_out, float *d_disp_low, unsigned char *d_img_low, unsigned char *d_img, int out_rows,
                         int out_cols, int in_rows, int in_cols, int elem_sz, float up, float sigma_color)
{
    if (!upsample_args_ok("d_disp_upsample", out_rows, out_cols, in_rows, in_cols, elem_sz, sigma_color)) return;
    float *o[1] = {d_disp_out};
    const float *dl[1] = {d_disp_low};
    const u8 *il[1] = {d_img_low}, *im[1] = {d_img};
    launch_disp_upsample(1, o, dl, il, im, upsample_table(sigma_color), out_rows, out_cols, in_rows, in_cols, elem_sz, up);
}
void stm_disp_upsample(float *disp_out, float *disp_low, unsigned char *img_low, unsigned char *img, int out_rows, int out_cols,
                       int in_rows, int in_cols, int elem_sz, float up_factor, float sigma_color)
{
    if (!upsample_args_ok("disp_upsample", out_rows, out_cols, in_rows, in_cols, elem_sz, sigma_color)) return;
    const size_t HW = (size_t)out_rows * out_cols, hw = (size_t)in_rows * in_cols;
    Workspace::begin((4 + (size_t)elem_sz) * (HW + hw) + 8192);
    float *dl = up(disp_low, hw), *o = Workspace::get<float>(HW);
    u8 *il = up(img_low, hw * elem_sz), *im = up(img, HW * elem_sz);
    float *ov[1] = {o};
    const float *dv[1] = {dl};
    const u8 *ilv[1] = {il}, *imv[1] = {im};
    launch_disp_upsample(1, ov, dv, ilv, imv, upsample_table(sigma_color), out_rows, out_cols, in_rows, in_cols, elem_sz, up_factor);
    down(disp_out, o, HW);
    sync();
}

// =============================================================== temporal disparity stabilisation
// (an addition, the reference has none: its video loop matches every frame on its own)
void stm_d_disp_temporal(float *d_disp, float *d_disp_prev, unsigned char *d_img, unsigned char *d_img_prev, int num_rows, int num_cols,
                         int elem_sz, float alpha, int thresh_color, float thresh_disp)
{
    if (!temporal_args_ok("d_disp_temporal", d_disp, d_disp_prev, num_rows, num_cols, elem_sz, alpha, thresh_color, thresh_disp)) return;
    float *c[1] = {d_disp};
    const float *q[1] = {d_disp_prev};
    const u8 *im[1] = {d_img}, *ip[1] = {d_img_prev};
    const size_t off[1] = {0};
    launch_disp_temporal(1, c, q, im, ip, off, num_rows, num_cols, num_cols, elem_sz, alpha, thresh_color, thresh_disp);
}
void stm_disp_temporal(float *disp, float *disp_prev, unsigned char *img, unsigned char *img_prev, int num_rows, int num_cols,
                       int elem_sz, float alpha, int thresh_color, float thresh_disp)
{
    if (!temporal_args_ok("disp_temporal", disp, disp_prev, num_rows, num_cols, elem_sz, alpha, thresh_color, thresh_disp)) return;
    const size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(2 * (4 + (size_t)elem_sz) * HW + 8192);
    float *c = up(disp, HW), *q = up(disp_prev, HW);
    u8 *im = up(img, HW * elem_sz), *ip = up(img_prev, HW * elem_sz);
    float *cv[1] = {c};
    const float *qv[1] = {q};
    const u8 *imv[1] = {im}, *ipv[1] = {ip};
    const size_t off[1] = {0};
    launch_disp_temporal(1, cv, qv, imv, ipv, off, num_rows, num_cols, num_cols, elem_sz, alpha, thresh_color, thresh_disp);
    down(disp, c, HW);
    sync();
}

// =============================================================== depth budget: the measurement as a stage
// (an addition, the reference has none: its views always span the camera baseline)
static bool depth_fit_args_ok(const char *fn, int num_rows, int num_cols, float disp_lo, float disp_hi, float max_gain, int clip_permille,
                              float rate)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return false;
    if ((size_t)num_rows * num_cols > 0x7fffffffu) // n = 2 H W is counted in 32 bits
        return STM_REJECT("num_rows, num_cols", "%s: num_rows * num_cols = %zu, must be below 2^31", fn, (size_t)num_rows * num_cols);
    return depth_auto_params_ok(fn, disp_lo, disp_hi, max_gain, clip_permille, rate);
}
// stm_d_depth_fit and stm_d_depth_fit_rect (d_rect null: the whole map), stm_depth_fit and stm_depth_fit_rect likewise
static void depth_fit_device(const char *fn, float *d_disp_l, float *d_disp_r, int num_rows, int num_cols, float disp_lo, float disp_hi,
                             float max_gain, int clip_permille, float rate, float *d_state, const int *d_rect)
{
    if (!depth_fit_args_ok(fn, num_rows, num_cols, disp_lo, disp_hi, max_gain, clip_permille, rate)) return;
    Workspace::begin(4096 * 4 + 8192);
    uint32_t *hist = Workspace::get<uint32_t>(4096);
    launch_depth_fit(d_state, hist, d_disp_l, d_disp_r, num_rows, num_cols, disp_lo, disp_hi, max_gain, clip_permille, rate, false, d_rect);
}
static void depth_fit_host(const char *fn, float *disp_l, float *disp_r, int num_rows, int num_cols, float disp_lo, float disp_hi, float max_gain,
                           int clip_permille, float rate, float *state, const int *rect)
{
    if (!depth_fit_args_ok(fn, num_rows, num_cols, disp_lo, disp_hi, max_gain, clip_permille, rate)) return;
    if (rect && !active_rect_ok(fn, rect, num_rows, num_cols)) return;
    const size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(8 * HW + 4096 * 4 + 8192);
    float *dl = up(disp_l, HW), *dr = up(disp_r, HW), *st = up(state, 4);
    const int *rc = rect ? up(rect, 4) : nullptr;
    uint32_t *hist = Workspace::get<uint32_t>(4096);
    launch_depth_fit(st, hist, dl, dr, num_rows, num_cols, disp_lo, disp_hi, max_gain, clip_permille, rate, false, rc);
    down(state, st, 4);
    sync();
}
void stm_d_depth_fit(float *d_disp_l, float *d_disp_r, int num_rows, int num_cols, float disp_lo, float disp_hi, float max_gain,
                     int clip_permille, float rate, float *d_state)
{
    depth_fit_device("d_depth_fit", d_disp_l, d_disp_r, num_rows, num_cols, disp_lo, disp_hi, max_gain, clip_permille, rate, d_state, nullptr);
}
void stm_d_depth_fit_rect(float *d_disp_l, float *d_disp_r, int num_rows, int num_cols, float disp_lo, float disp_hi, float max_gain,
                          int clip_permille, float rate, float *d_state, const int *d_rect)
{
    depth_fit_device("d_depth_fit_rect", d_disp_l, d_disp_r, num_rows, num_cols, disp_lo, disp_hi, max_gain, clip_permille, rate, d_state, d_rect);
}
void stm_depth_fit(float *disp_l, float *disp_r, int num_rows, int num_cols, float disp_lo, float disp_hi, float max_gain,
                   int clip_permille, float rate, float *state)
{
    depth_fit_host("depth_fit", disp_l, disp_r, num_rows, num_cols, disp_lo, disp_hi, max_gain, clip_permille, rate, state, nullptr);
}
void stm_depth_fit_rect(float *disp_l, float *disp_r, int num_rows, int num_cols, float disp_lo, float disp_hi, float max_gain,
                        int clip_permille, float rate, float *state, const int *rect)
{
    depth_fit_host("depth_fit_rect", disp_l, disp_r, num_rows, num_cols, disp_lo, disp_hi, max_gain, clip_permille, rate, state, rect);
}

// =============================================================== overlay placement: the measurement as a stage
// (an addition, the reference has no overlay)
// the numbers of an overlay fit under the names the four entries give them, and those names in the record's order (as STM_FRAME_PARAMS)
struct OverlayFitArgs {
    int num_rows, num_cols, ov_rows, ov_cols, x0, y0, view_rows, view_cols;
    float gain, conv;
    int near_permille;
    float margin;
    int pad;
    float limit_lo, limit_hi, rate_near, rate_far;
    int restart;
};
#define STM_OVERLAY_FIT_PARAMS \
    num_rows, num_cols, ov_rows, ov_cols, x0, y0, view_rows, view_cols, gain, conv, near_permille, margin, pad, limit_lo, limit_hi, rate_near, rate_far, restart
static bool overlay_fit_args_ok(const char *fn, const unsigned char *overlay, bool words, const OverlayFitArgs &a)
{
    if (!args_ok(fn, {{"num_rows", a.num_rows, 1}, {"num_cols", a.num_cols, 1}, {"view_rows", a.view_rows, 1}, {"view_cols", a.view_cols, 1}}))
        return false;
    if (!overlay_fit_size_ok(fn, a.num_rows, a.num_cols)) return false;
    if (!overlay_params_ok(fn, overlay, words, a.ov_rows, a.ov_cols, a.x0, a.y0, 0.0f)) return false;
    if (!overlay) return STM_REJECT("overlay", "%s: the overlay is null", fn);
    return depth_params_ok(fn, 1, a.gain, a.conv) &&
           overlay_auto_params_ok(fn, a.near_permille, a.margin, a.pad, a.limit_lo, a.limit_hi, a.rate_near, a.rate_far);
}
// the fit's launch on device buffers, shared by both flavours
static void overlay_fit_launch(float *st, uint32_t *ws, const float *dl, const float *dr, const u8 *ov, const OverlayFitArgs &a, const int *cut_state,
                               const int *d_rect)
{
    const OverlayAuto oa = {1, a.near_permille, a.margin, a.pad, a.limit_lo, a.limit_hi, a.rate_near, a.rate_far, st};
    launch_overlay_fit(st, ws, dl, dr, a.num_rows, a.num_cols, ov, a.ov_rows, a.ov_cols, a.x0, a.y0, a.view_rows, a.view_cols, a.gain, a.conv, nullptr,
                       oa, a.restart != 0, false, cut_state, d_rect);
}
// stm_d_overlay_fit and stm_d_overlay_fit_rect (d_rect null: the whole map), stm_overlay_fit and stm_overlay_fit_rect likewise
static void overlay_fit_device(const char *fn, float *d_disp_l, float *d_disp_r, const unsigned char *d_overlay, const OverlayFitArgs &a,
                               float *d_state, const int *d_cut_state, const int *d_rect)
{
    if (!overlay_fit_args_ok(fn, d_overlay, true, a)) return;
    Workspace::begin(OVERLAY_FIT_WS_WORDS * 4 + 8192);
    uint32_t *ws = Workspace::get<uint32_t>(OVERLAY_FIT_WS_WORDS);
    overlay_fit_launch(d_state, ws, d_disp_l, d_disp_r, d_overlay, a, d_cut_state, d_rect);
}
static void overlay_fit_host(const char *fn, float *disp_l, float *disp_r, const unsigned char *overlay, const OverlayFitArgs &a, float *state,
                             const int *rect)
{
    if (!overlay_fit_args_ok(fn, overlay, false, a)) return;
    if (rect && !active_rect_ok(fn, rect, a.num_rows, a.num_cols)) return;
    const size_t HW = (size_t)a.num_rows * a.num_cols, ov_sz = (size_t)a.ov_rows * a.ov_cols * 4;
    Workspace::begin(8 * HW + ov_sz + OVERLAY_FIT_WS_WORDS * 4 + 8192);
    float *dl = up(disp_l, HW), *dr = up(disp_r, HW), *st = up(state, 4);
    const u8 *o = up((unsigned char *)overlay, ov_sz);
    const int *rc = rect ? up(rect, 4) : nullptr;
    uint32_t *ws = Workspace::get<uint32_t>(OVERLAY_FIT_WS_WORDS);
    overlay_fit_launch(st, ws, dl, dr, o, a, nullptr, rc);
    down(state, st, 4);
    sync();
}
void stm_d_overlay_fit(float *d_disp_l, float *d_disp_r, int num_rows, int num_cols, const unsigned char *d_overlay, int ov_rows, int ov_cols,
                       int x0, int y0, int view_rows, int view_cols, float gain, float conv, int near_permille, float margin, int pad,
                       float limit_lo, float limit_hi, float rate_near, float rate_far, int restart, float *d_state, const int *d_cut_state)
{
    overlay_fit_device("d_overlay_fit", d_disp_l, d_disp_r, d_overlay, {STM_OVERLAY_FIT_PARAMS}, d_state, d_cut_state, nullptr);
}
void stm_d_overlay_fit_rect(float *d_disp_l, float *d_disp_r, int num_rows, int num_cols, const unsigned char *d_overlay, int ov_rows,
                            int ov_cols, int x0, int y0, int view_rows, int view_cols, float gain, float conv, int near_permille, float margin,
                            int pad, float limit_lo, float limit_hi, float rate_near, float rate_far, int restart, float *d_state,
                            const int *d_cut_state, const int *d_rect)
{
    overlay_fit_device("d_overlay_fit_rect", d_disp_l, d_disp_r, d_overlay, {STM_OVERLAY_FIT_PARAMS}, d_state, d_cut_state, d_rect);
}
void stm_overlay_fit(float *disp_l, float *disp_r, int num_rows, int num_cols, const unsigned char *overlay, int ov_rows, int ov_cols, int x0,
                     int y0, int view_rows, int view_cols, float gain, float conv, int near_permille, float margin, int pad, float limit_lo,
                     float limit_hi, float rate_near, float rate_far, int restart, float *state)
{
    overlay_fit_host("overlay_fit", disp_l, disp_r, overlay, {STM_OVERLAY_FIT_PARAMS}, state, nullptr);
}
void stm_overlay_fit_rect(float *disp_l, float *disp_r, int num_rows, int num_cols, const unsigned char *overlay, int ov_rows, int ov_cols,
                          int x0, int y0, int view_rows, int view_cols, float gain, float conv, int near_permille, float margin, int pad,
                          float limit_lo, float limit_hi, float rate_near, float rate_far, int restart, float *state, const int *rect)
{
    overlay_fit_host("overlay_fit_rect", disp_l, disp_r, overlay, {STM_OVERLAY_FIT_PARAMS}, state, rect);
}

// =============================================================== vertical alignment: the field applied and measured as stages
// (an addition, the reference has none: it takes rectified pairs)
static bool align_rows_args_ok(const char *fn, const unsigned char *img_out, const unsigned char *img, int num_rows, int num_cols, int elem_sz,
                               float a, float b, float c)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}})) return false;
    if (!align_params_ok(fn, 1, a, b, c)) return false;
    if (!ptrs_ok(fn, {{"img_out", img_out}, {"img", img}})) return false;
    const size_t bytes = (size_t)num_rows * num_cols * elem_sz;
    if (bytes_overlap(img_out, bytes, img, bytes)) return STM_REJECT("img_out", "%s: img_out must not overlap img", fn); // a pixel's taps are other rows' outputs
    return true;
}
void stm_d_align_rows(unsigned char *d_img_out, const unsigned char *d_img, int num_rows, int num_cols, int elem_sz, float a, float b, float c)
{
    if (!align_rows_args_ok("d_align_rows", d_img_out, d_img, num_rows, num_cols, elem_sz, a, b, c)) return;
    launch_align_frame(d_img_out, nullptr, d_img, num_rows, num_cols, elem_sz, a, b, c, nullptr);
}
void stm_align_rows(unsigned char *img_out, const unsigned char *img, int num_rows, int num_cols, int elem_sz, float a, float b, float c)
{
    if (!align_rows_args_ok("align_rows", img_out, img, num_rows, num_cols, elem_sz, a, b, c)) return;
    const size_t IMG = (size_t)num_rows * num_cols * elem_sz;
    Workspace::begin(2 * IMG + 8192);
    const u8 *i = up(img, IMG);
    u8 *o = Workspace::get<u8>(IMG);
    if (elem_sz > 3) STM_CHECK(hipMemsetAsync(o, 0, IMG, stream())); // bytes past the third come back 0
    launch_align_frame(o, nullptr, i, num_rows, num_cols, elem_sz, a, b, c, nullptr);
    down(img_out, o, IMG);
    sync();
}
// =============================================================== rectification: one image through one record, and the test tap
// (include/stm_rectify.h; an addition, the reference has none: it takes rectified pairs)
static bool rectify_dims_ok(const char *fn, int num_rows, int num_cols)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return false;
    if (num_rows > 16384) return STM_REJECT("num_rows", "%s: num_rows = %d, must be <= 16384", fn, num_rows);
    if (num_cols > 16384) return STM_REJECT("num_cols", "%s: num_cols = %d, must be <= 16384", fn, num_cols);
    return true;
}
static bool rectify_args_ok(const char *fn, const unsigned char *img_out, const unsigned char *img, const float *rec18, int num_rows,
                            int num_cols, int elem_sz, int border)
{
    if (!rectify_dims_ok(fn, num_rows, num_cols) || !args_ok(fn, {{"elem_sz", elem_sz, 3}})) return false;
    if (!ptrs_ok(fn, {{"img_out", img_out}, {"img", img}, {"rec18", rec18}})) return false;
    if (!rectify_params_ok(fn, rec18, border)) return false;
    const size_t bytes = (size_t)num_rows * num_cols * elem_sz;
    if (bytes_overlap(img_out, bytes, img, bytes)) return STM_REJECT("img_out", "%s: img_out must not overlap img", fn); // a pixel's taps are other pixels' outputs
    return true;
}
void stm_d_rectify(unsigned char *d_img_out, const unsigned char *d_img, const float *rec18, int num_rows, int num_cols, int elem_sz, int border)
{
    if (!rectify_args_ok("d_rectify", d_img_out, d_img, rec18, num_rows, num_cols, elem_sz, border)) return;
    launch_rectify_frame(d_img_out, nullptr, d_img, num_rows, num_cols, elem_sz, (const float (*)[18])rec18, border);
}
void stm_rectify(unsigned char *img_out, const unsigned char *img, const float *rec18, int num_rows, int num_cols, int elem_sz, int border)
{
    if (!rectify_args_ok("rectify", img_out, img, rec18, num_rows, num_cols, elem_sz, border)) return;
    const size_t IMG = (size_t)num_rows * num_cols * elem_sz;
    Workspace::begin(2 * IMG + 8192);
    const u8 *i = up(img, IMG);
    u8 *o = Workspace::get<u8>(IMG);
    if (elem_sz > 3) STM_CHECK(hipMemsetAsync(o, 0, IMG, stream())); // bytes past the third come back 0
    launch_rectify_frame(o, nullptr, i, num_rows, num_cols, elem_sz, (const float (*)[18])rec18, border);
    down(img_out, o, IMG);
    sync();
}
void stm_rectify_coords(int *quv, const float *rec18, int num_rows, int num_cols)
{
    const char *fn = "rectify_coords";
    if (!rectify_dims_ok(fn, num_rows, num_cols)) return;
    if (!ptrs_ok(fn, {{"quv", quv}, {"rec18", rec18}}) || !rectify_params_ok(fn, rec18, 0)) return;
    const size_t n = (size_t)num_rows * num_cols * 2;
    Workspace::begin(n * 4 + 8192);
    int *d = Workspace::get<int>(n);
    launch_rectify_coords(d, num_rows, num_cols, rec18);
    down(quv, d, n);
    sync();
}
static bool align_fit_args_ok(const char *fn, const unsigned char *img_l, const unsigned char *img_r, int num_rows, int num_cols, int elem_sz,
                              int radius, float rate, const float *state)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}})) return false;
    if (!align_size_ok(fn, num_rows, num_cols) || !align_auto_params_ok(fn, radius, rate)) return false;
    return ptrs_ok(fn, {{"img_l", img_l}, {"img_r", img_r}, {"state", state}});
}
void stm_d_align_fit(const unsigned char *d_img_l, const unsigned char *d_img_r, int num_rows, int num_cols, int elem_sz, int radius,
                     float rate, float *d_state, int *d_valid_blocks, unsigned int *d_profiles, unsigned int *d_sad)
{
    if (!align_fit_args_ok("d_align_fit", d_img_l, d_img_r, num_rows, num_cols, elem_sz, radius, rate, d_state)) return;
    Workspace::begin((align_profile_words(num_rows) + align_sad_words(radius)) * 4 + 8192);
    uint32_t *prof = d_profiles ? d_profiles : Workspace::get<uint32_t>(align_profile_words(num_rows));
    uint32_t *sad = d_sad ? d_sad : Workspace::get<uint32_t>(align_sad_words(radius));
    launch_align_measure(d_state, d_valid_blocks, prof, sad, nullptr, d_img_l, d_img_r, num_rows, num_cols, elem_sz, radius, rate, false);
}
int stm_align_fit(const unsigned char *img_l, const unsigned char *img_r, int num_rows, int num_cols, int elem_sz, int radius, float rate,
                  float *state)
{
    if (!align_fit_args_ok("align_fit", img_l, img_r, num_rows, num_cols, elem_sz, radius, rate, state)) return -1;
    const size_t IMG = (size_t)num_rows * num_cols * elem_sz;
    Workspace::begin(2 * IMG + (align_profile_words(num_rows) + align_sad_words(radius)) * 4 + 8192);
    const u8 *l = up(img_l, IMG), *r = up(img_r, IMG);
    float *st = up(state, 4);
    int *nv = Workspace::get<int>(1);
    uint32_t *prof = Workspace::get<uint32_t>(align_profile_words(num_rows)), *sad = Workspace::get<uint32_t>(align_sad_words(radius));
    launch_align_measure(st, nv, prof, sad, nullptr, l, r, num_rows, num_cols, elem_sz, radius, rate, false);
    int count = -1;
    down(state, st, 4);
    down(&count, nv, 1);
    sync();
    return failed() ? -1 : count;
}

// =============================================================== colour balance between the eyes: measured and applied as stages
// (an addition, the reference has none: it takes graded pairs)
static bool balance_fit_args_ok(const char *fn, const unsigned char *img_l, const unsigned char *img_r, int num_rows, int num_cols, int elem_sz,
                                int max_shift, float rate, const int *state)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}})) return false;
    if (!balance_size_ok(fn, num_rows, num_cols) || !balance_auto_params_ok(fn, max_shift, rate)) return false;
    return ptrs_ok(fn, {{"img_l", img_l}, {"img_r", img_r}, {"state", state}});
}
void stm_d_balance_fit(const unsigned char *d_img_l, const unsigned char *d_img_r, int num_rows, int num_cols, int elem_sz, int max_shift,
                       float rate, int *d_state, unsigned int *d_hist)
{
    if (!balance_fit_args_ok("d_balance_fit", d_img_l, d_img_r, num_rows, num_cols, elem_sz, max_shift, rate, d_state)) return;
    Workspace::begin(BALANCE_HIST_WORDS * 4 + 8192);
    uint32_t *hist = d_hist ? d_hist : Workspace::get<uint32_t>(BALANCE_HIST_WORDS);
    launch_balance_measure(d_state, hist, nullptr, d_img_l, d_img_r, num_rows, num_cols, elem_sz, max_shift, balance_rate_q(rate), false);
}
int stm_balance_fit(const unsigned char *img_l, const unsigned char *img_r, int num_rows, int num_cols, int elem_sz, int max_shift, float rate,
                    int *state)
{
    if (!balance_fit_args_ok("balance_fit", img_l, img_r, num_rows, num_cols, elem_sz, max_shift, rate, state)) return -1;
    const size_t IMG = (size_t)num_rows * num_cols * elem_sz;
    Workspace::begin(2 * IMG + (BALANCE_HIST_WORDS + BALANCE_STATE_WORDS) * 4 + 8192);
    const u8 *l = up(img_l, IMG), *r = up(img_r, IMG);
    int *st = up(state, BALANCE_STATE_WORDS);
    uint32_t *hist = Workspace::get<uint32_t>(BALANCE_HIST_WORDS);
    launch_balance_measure(st, hist, nullptr, l, r, num_rows, num_cols, elem_sz, max_shift, balance_rate_q(rate), false);
    down(state, st, BALANCE_STATE_WORDS);
    sync();
    return failed() ? -1 : 0;
}
static bool balance_apply_args_ok(const char *fn, const unsigned char *img_out, const unsigned char *img, int num_rows, int num_cols, int elem_sz,
                                  const unsigned char *lut768, const int *state)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}})) return false;
    if (!ptrs_ok(fn, {{"img_out", img_out}, {"img", img}})) return false;
    if ((lut768 != nullptr) == (state != nullptr))
        return STM_REJECT("lut768, state", "%s: exactly one of lut768 and state must be given", fn);
    const size_t bytes = (size_t)num_rows * num_cols * elem_sz;
    if (bytes_overlap(img_out, bytes, img, bytes)) return STM_REJECT("img_out", "%s: img_out must not overlap img", fn);
    return true;
}
void stm_d_balance_apply(unsigned char *d_img_out, const unsigned char *d_img, int num_rows, int num_cols, int elem_sz,
                         const unsigned char *lut768, const int *d_state)
{
    if (!balance_apply_args_ok("d_balance_apply", d_img_out, d_img, num_rows, num_cols, elem_sz, lut768, d_state)) return;
    launch_balance_frame(d_img_out, nullptr, d_img, num_rows, num_cols, elem_sz, lut768, d_state);
}
void stm_balance_apply(unsigned char *img_out, const unsigned char *img, int num_rows, int num_cols, int elem_sz, const unsigned char *lut768,
                       const int *state)
{
    if (!balance_apply_args_ok("balance_apply", img_out, img, num_rows, num_cols, elem_sz, lut768, state)) return;
    const size_t IMG = (size_t)num_rows * num_cols * elem_sz;
    Workspace::begin(2 * IMG + BALANCE_STATE_WORDS * 4 + 8192);
    const u8 *i = up(img, IMG);
    const int *st = state ? up(state, BALANCE_STATE_WORDS) : nullptr;
    u8 *o = Workspace::get<u8>(IMG);
    if (elem_sz > 3) STM_CHECK(hipMemsetAsync(o, 0, IMG, stream())); // bytes past the third come back 0
    launch_balance_frame(o, nullptr, i, num_rows, num_cols, elem_sz, lut768, st);
    down(img_out, o, IMG);
    sync();
}

// =============================================================== shot changes: the detector as a stage
// (an addition, the reference has none: it keeps no state from frame to frame)
static bool cut_args_ok(const char *fn, const unsigned char *img_l, int num_rows, int num_cols, int elem_sz, int thresh_permille, int min_gap,
                        const int *state)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 4}, {"num_cols", num_cols, 4}, {"elem_sz", elem_sz, 3}})) return false;
    if (!cut_size_ok(fn, num_rows, num_cols) || !cut_params_ok(fn, thresh_permille, min_gap)) return false;
    return ptrs_ok(fn, {{"img_l", img_l}, {"state", state}});
}
void stm_d_cut_detect(const unsigned char *d_img_l, int num_rows, int num_cols, int elem_sz, int thresh_permille, int min_gap, int *d_state,
                      void *d_reset0, void *d_reset1, void *d_reset2, unsigned int *d_sig)
{
    if (!cut_args_ok("d_cut_detect", d_img_l, num_rows, num_cols, elem_sz, thresh_permille, min_gap, d_state)) return;
    Workspace::begin(CUT_SIG_WORDS * 4 + 8192);
    uint32_t *sig = d_sig ? d_sig : Workspace::get<uint32_t>(CUT_SIG_WORDS);
    launch_cut_detect(d_state, sig, nullptr, d_img_l, num_rows, num_cols, elem_sz, thresh_permille, min_gap, d_reset0, d_reset1, d_reset2);
}
int stm_cut_detect(const unsigned char *img_l, int num_rows, int num_cols, int elem_sz, int thresh_permille, int min_gap, int *state)
{
    if (!cut_args_ok("cut_detect", img_l, num_rows, num_cols, elem_sz, thresh_permille, min_gap, state)) return -1;
    const size_t IMG = (size_t)num_rows * num_cols * elem_sz;
    Workspace::begin(IMG + (CUT_SIG_WORDS + CUT_STATE_WORDS) * 4 + 8192);
    const u8 *l = up(img_l, IMG);
    int *st = up(state, CUT_STATE_WORDS);
    uint32_t *sig = Workspace::get<uint32_t>(CUT_SIG_WORDS);
    launch_cut_detect(st, sig, nullptr, l, num_rows, num_cols, elem_sz, thresh_permille, min_gap, nullptr, nullptr, nullptr);
    down(state, st, CUT_STATE_WORDS);
    sync();
    return failed() ? -1 : state[1];
}

// =============================================================== active picture area: measured and applied as stages
// (an addition, the reference has none: it matches and measures black bars as if they were picture)
static bool active_args_ok(const char *fn, const unsigned char *img_l, int num_rows, int num_cols, int elem_sz, int thresh_luma, int lit_permille,
                           int max_bar_permille, int hold, const int *state)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}})) return false;
    if (!active_size_ok(fn, num_rows, num_cols) || !active_auto_params_ok(fn, thresh_luma, lit_permille, max_bar_permille, hold)) return false;
    return ptrs_ok(fn, {{"img_l", img_l}, {"state", state}});
}
void stm_d_active_detect(const unsigned char *d_img_l, int num_rows, int num_cols, int elem_sz, int thresh_luma, int lit_permille,
                         int max_bar_permille, int hold, int restart, int *d_state, const int *d_cut_state, unsigned int *d_counts)
{
    if (!active_args_ok("d_active_detect", d_img_l, num_rows, num_cols, elem_sz, thresh_luma, lit_permille, max_bar_permille, hold, d_state)) return;
    const size_t words = (size_t)num_rows + num_cols;
    Workspace::begin(words * 4 + 8192);
    uint32_t *counts = d_counts ? d_counts : Workspace::get<uint32_t>(words);
    launch_active_detect(d_state, counts, nullptr, d_img_l, num_rows, num_cols, elem_sz, thresh_luma, lit_permille, max_bar_permille, hold,
                         restart != 0, d_cut_state);
}
int stm_active_detect(const unsigned char *img_l, int num_rows, int num_cols, int elem_sz, int thresh_luma, int lit_permille, int max_bar_permille,
                      int hold, int restart, int *state)
{
    if (!active_args_ok("active_detect", img_l, num_rows, num_cols, elem_sz, thresh_luma, lit_permille, max_bar_permille, hold, state)) return -1;
    const size_t IMG = (size_t)num_rows * num_cols * elem_sz, words = (size_t)num_rows + num_cols;
    Workspace::begin(IMG + (words + ACTIVE_STATE_WORDS) * 4 + 8192);
    const u8 *l = up(img_l, IMG);
    int *st = up(state, ACTIVE_STATE_WORDS);
    uint32_t *counts = Workspace::get<uint32_t>(words);
    launch_active_detect(st, counts, nullptr, l, num_rows, num_cols, elem_sz, thresh_luma, lit_permille, max_bar_permille, hold, restart != 0, nullptr);
    down(state, st, ACTIVE_STATE_WORDS);
    sync();
    return failed() ? -1 : state[5];
}
static bool active_fill_args_ok(const char *fn, const float *disp, int num_rows, int num_cols)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}})) return false;
    return ptrs_ok(fn, {{"disp", disp}});
}
void stm_d_active_fill(float *d_disp, int num_rows, int num_cols, const int *d_rect, float value)
{
    if (!active_fill_args_ok("d_active_fill", d_disp, num_rows, num_cols)) return;
    if (!d_rect) return; // the whole map is picture: nothing to write
    float *m[1] = {d_disp};
    launch_active_fill(1, m, num_rows, num_cols, d_rect, value);
}
void stm_active_fill(float *disp, int num_rows, int num_cols, const int *rect, float value)
{
    if (!active_fill_args_ok("active_fill", disp, num_rows, num_cols)) return;
    if (!rect) return;
    if (!active_rect_ok("active_fill", rect, num_rows, num_cols)) return;
    const size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(4 * HW + 8192);
    float *d = up(disp, HW);
    const int *rc = up(rect, 4);
    float *m[1] = {d};
    launch_active_fill(1, m, num_rows, num_cols, rc, value);
    down(disp, d, HW);
    sync();
}

// =============================================================== view antialiasing: the prefilter as a stage
// (an addition, the reference has none: its views are pinhole images whatever the lens shows of them)
static bool prefilter_args_ok(const char *fn, const unsigned char *img_out, const unsigned char *img, const float *disp, int num_rows,
                              int num_cols, int elem_sz, int num_views, float strength, int max_radius, float gate, float gain, float conv)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols", num_cols, 1}, {"elem_sz", elem_sz, 3}, {"num_views", num_views, 2}})) return false;
    if (!antialias_params_ok(fn, strength, max_radius, gate)) return false;
    if (!depth_params_ok(fn, 1, gain, conv)) return false;
    if (!ptrs_ok(fn, {{"img_out", img_out}, {"img", img}, {"disp", disp}})) return false;
    const size_t bytes = (size_t)num_rows * num_cols * elem_sz;
    if (bytes_overlap(img_out, bytes, img, bytes)) return STM_REJECT("img_out", "%s: img_out must not overlap img", fn); // a pixel's taps are its neighbours' inputs
    return true;
}
void stm_d_view_prefilter(unsigned char *d_img_out, const unsigned char *d_img, const float *d_disp, int num_rows, int num_cols, int elem_sz,
                          int num_views, float strength, int max_radius, float gate, float gain, float conv)
{
    if (!prefilter_args_ok("d_view_prefilter", d_img_out, d_img, d_disp, num_rows, num_cols, elem_sz, num_views, strength, max_radius, gate, gain,
                           conv))
        return;
    launch_view_prefilter(1, &d_img_out, &d_img, &d_disp, num_rows, num_cols, elem_sz, num_views, strength, max_radius, gate, gain, conv, nullptr);
}
void stm_view_prefilter(unsigned char *img_out, const unsigned char *img, const float *disp, int num_rows, int num_cols, int elem_sz,
                        int num_views, float strength, int max_radius, float gate, float gain, float conv)
{
    if (!prefilter_args_ok("view_prefilter", img_out, img, disp, num_rows, num_cols, elem_sz, num_views, strength, max_radius, gate, gain, conv))
        return;
    const size_t HW = (size_t)num_rows * num_cols;
    Workspace::begin(2 * HW * elem_sz + 4 * HW + 8192);
    const u8 *i = up(img, HW * elem_sz);
    const float *d = up(disp, HW);
    u8 *o = Workspace::get<u8>(HW * elem_sz);
    if (elem_sz > 3) STM_CHECK(hipMemsetAsync(o, 0, HW * elem_sz, stream())); // bytes past the third come back 0
    launch_view_prefilter(1, &o, &i, &d, num_rows, num_cols, elem_sz, num_views, strength, max_radius, gate, gain, conv, nullptr);
    down(img_out, o, HW * elem_sz);
    sync();
}

// =============================================================== mux
void stm_d_mux_multiview(unsigned char **d_views, unsigned char *d_out_data, int num_views, float angle, int in_rows,
                         int in_cols, int out_rows, int out_cols, int elem_sz)
{
    if (!args_ok("d_mux_multiview", {{"num_views", num_views, 2}, {"in_rows", in_rows, 1}, {"in_cols", in_cols, 1},
                                     {"out_rows", out_rows, 1}, {"out_cols", out_cols, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    core_mux((const u8 *const *)d_views, d_out_data, num_views, angle, in_rows, in_cols, out_rows, out_cols, elem_sz, 2); // :148-151
}
void stm_mux_multiview(unsigned char **views, unsigned char *out_data, int num_views, float angle, int in_rows, int in_cols,
                       int out_rows, int out_cols, int elem_sz)
{
    if (!args_ok("mux_multiview", {{"num_views", num_views, 2}, {"in_rows", in_rows, 1}, {"in_cols", in_cols, 1},
                                   {"out_rows", out_rows, 1}, {"out_cols", out_cols, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    size_t in_sz = (size_t)in_rows * in_cols * elem_sz, out_sz = (size_t)out_rows * out_cols * elem_sz;
    Workspace::begin(num_views * (in_sz + 256) + out_sz + 8192);
    u8 **dv = up_views(views, num_views, in_sz);
    u8 *o = Workspace::get<u8>(out_sz);
    STM_CHECK(hipMemsetAsync(o, 0, out_sz, stream()));
    int variant = (out_rows % num_views == 0) ? 2 : 1; // d_mux_multiview.cu:184-192
    core_mux((const u8 *const *)dv, o, num_views, angle, in_rows, in_cols, out_rows, out_cols, elem_sz, variant);
    down(out_data, o, out_sz);
    sync();
}

// the interlacer under a lens geometry (an addition: the reference's interlacer fits one panel); modes 1 and 2 (stm_hip.h)
void stm_d_mux_multiview_lens(unsigned char **d_views, unsigned char *d_out_data, int num_views, int mode, double pitch, double slope,
                              double centre, int in_rows, int in_cols, int out_rows, int out_cols, int elem_sz)
{
    const char *fn = "d_mux_multiview_lens";
    if (!args_ok(fn, {{"num_views", num_views, 2}, {"in_rows", in_rows, 1}, {"in_cols", in_cols, 1}, {"out_rows", out_rows, 1},
                      {"out_cols", out_cols, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    if (!lens_params_ok(fn, mode, 1, 2, pitch, slope, centre)) return;
    launch_mux_lens((const u8 *const *)d_views, d_out_data, num_views, Lens{mode, pitch, slope, centre}, in_rows, in_cols, out_rows,
                    out_cols, elem_sz);
}
void stm_mux_multiview_lens(unsigned char **views, unsigned char *out_data, int num_views, int mode, double pitch, double slope,
                            double centre, int in_rows, int in_cols, int out_rows, int out_cols, int elem_sz)
{
    const char *fn = "mux_multiview_lens";
    if (!args_ok(fn, {{"num_views", num_views, 2}, {"in_rows", in_rows, 1}, {"in_cols", in_cols, 1}, {"out_rows", out_rows, 1},
                      {"out_cols", out_cols, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    if (!lens_params_ok(fn, mode, 1, 2, pitch, slope, centre)) return;
    size_t in_sz = (size_t)in_rows * in_cols * elem_sz, out_sz = (size_t)out_rows * out_cols * elem_sz;
    Workspace::begin(num_views * (in_sz + 256) + out_sz + 8192);
    u8 **dv = up_views(views, num_views, in_sz);
    u8 *o = Workspace::get<u8>(out_sz);
    STM_CHECK(hipMemsetAsync(o, 0, out_sz, stream())); // bytes past a pixel's third come back 0
    launch_mux_lens((const u8 *const *)dv, o, num_views, Lens{mode, pitch, slope, centre}, in_rows, in_cols, out_rows, out_cols, elem_sz);
    down(out_data, o, out_sz);
    sync();
}

// the views tiled into one frame (an addition; stm_hip.h): the quilt as a stage, filter 0 or 1
void stm_d_quilt_multiview(unsigned char **d_views, unsigned char *d_out_data, int num_views, int tiles_x, int tiles_y, int order, int filter,
                           int in_rows, int in_cols, int out_rows, int out_cols, int elem_sz)
{
    const char *fn = "d_quilt_multiview";
    if (!args_ok(fn, {{"num_views", num_views, 2}, {"in_rows", in_rows, 1}, {"in_cols", in_cols, 1}, {"out_rows", out_rows, 1},
                      {"out_cols", out_cols, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    if (!layout_params_ok(fn, 1, tiles_x, tiles_y, order, filter)) return;
    const Layout lo = {1, tiles_x, tiles_y, order, filter};
    if (!quilt_args_ok(fn, lo, num_views, in_rows, in_cols, out_rows, out_cols, "num_views", "out_rows", "out_cols")) return;
    launch_quilt((const u8 *const *)d_views, d_out_data, num_views, lo, in_rows, in_cols, out_rows, out_cols, elem_sz);
}
void stm_quilt_multiview(unsigned char **views, unsigned char *out_data, int num_views, int tiles_x, int tiles_y, int order, int filter,
                         int in_rows, int in_cols, int out_rows, int out_cols, int elem_sz)
{
    const char *fn = "quilt_multiview";
    if (!args_ok(fn, {{"num_views", num_views, 2}, {"in_rows", in_rows, 1}, {"in_cols", in_cols, 1}, {"out_rows", out_rows, 1},
                      {"out_cols", out_cols, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    if (!layout_params_ok(fn, 1, tiles_x, tiles_y, order, filter)) return;
    const Layout lo = {1, tiles_x, tiles_y, order, filter};
    if (!quilt_args_ok(fn, lo, num_views, in_rows, in_cols, out_rows, out_cols, "num_views", "out_rows", "out_cols")) return;
    size_t in_sz = (size_t)in_rows * in_cols * elem_sz, out_sz = (size_t)out_rows * out_cols * elem_sz;
    Workspace::begin(num_views * (in_sz + 256) + out_sz + 8192);
    u8 **dv = up_views(views, num_views, in_sz);
    u8 *o = Workspace::get<u8>(out_sz);
    STM_CHECK(hipMemsetAsync(o, 0, out_sz, stream())); // bytes past a pixel's third come back 0
    launch_quilt((const u8 *const *)dv, o, num_views, lo, in_rows, in_cols, out_rows, out_cols, elem_sz);
    down(out_data, o, out_sz);
    sync();
}

// an overlay composited into a finished frame (an addition; stm_hip.h).  The screen of both flavours: the overlay's own arguments
// (words: the device flavour reads a pixel as one aligned word; the host flavour copies into an aligned buffer), then the frame's
// geometry under the stage's lens and layout rules; false with the error recorded
static bool overlay_stage_ok(const char *fn, const unsigned char *overlay, bool words, int ov_rows, int ov_cols, int x0, int y0, float disparity,
                             int num_views, int lens_mode, double pitch, double slope, double centre, int layout, int tiles_x, int tiles_y,
                             int order, int out_rows, int out_cols, int elem_sz)
{
    if (!args_ok(fn, {{"num_views", num_views, 2}, {"out_rows", out_rows, 1}, {"out_cols", out_cols, 1}, {"elem_sz", elem_sz, 3}})) return false;
    if (!overlay_params_ok(fn, overlay, words, ov_rows, ov_cols, x0, y0, disparity)) return false;
    if (!overlay) return STM_REJECT("overlay", "%s: the overlay is null", fn);
    if (!lens_params_ok(fn, lens_mode, 0, 3, pitch, slope, centre)) return false;
    if (!layout_params_ok(fn, layout, tiles_x, tiles_y, order, 0)) return false;
    if (layout == 0) return true;
    if (!overlay_tiles_ok(fn, Layout{1, tiles_x, tiles_y, order, 0}, num_views)) return false;
    if (lens_mode != 0)
        return STM_REJECT("layout, lens_mode", "%s: layout 1 (quilt) together with lens mode %d: a quilt is not interlaced, set one of them to 0", fn,
                          lens_mode);
    return quilt_args_ok(fn, Layout{1, tiles_x, tiles_y, order, 0}, num_views, 1, 1, out_rows, out_cols, "num_views", "out_rows", "out_cols");
}
void stm_d_mux_overlay(unsigned char *d_frame, const unsigned char *d_overlay, int ov_rows, int ov_cols, int x0, int y0, float disparity,
                       int num_views, float angle, int lens_mode, double pitch, double slope, double centre, int layout, int tiles_x,
                       int tiles_y, int order, int out_rows, int out_cols, int elem_sz)
{
    if (!overlay_stage_ok("d_mux_overlay", d_overlay, true, ov_rows, ov_cols, x0, y0, disparity, num_views, lens_mode, pitch, slope, centre, layout,
                          tiles_x, tiles_y, order, out_rows, out_cols, elem_sz))
        return;
    frame_overlay(d_frame, Overlay{1, d_overlay, ov_rows, ov_cols, x0, y0, disparity},
                  lens_mode == 0 ? Lens{0, 0.0, 0.0, 0.0} : Lens{lens_mode, pitch, slope, centre},
                  layout == 0 ? Layout{0, 1, 1, 0, 0} : Layout{1, tiles_x, tiles_y, order, 0}, num_views, angle, out_rows, out_cols, elem_sz);
}
void stm_mux_overlay(unsigned char *frame, const unsigned char *overlay, int ov_rows, int ov_cols, int x0, int y0, float disparity,
                     int num_views, float angle, int lens_mode, double pitch, double slope, double centre, int layout, int tiles_x,
                     int tiles_y, int order, int out_rows, int out_cols, int elem_sz)
{
    if (!overlay_stage_ok("mux_overlay", overlay, false, ov_rows, ov_cols, x0, y0, disparity, num_views, lens_mode, pitch, slope, centre, layout,
                          tiles_x, tiles_y, order, out_rows, out_cols, elem_sz))
        return;
    if (layout == 0 && lens_mode == 0 && !mux_geom_ok(num_views, angle, elem_sz, nullptr, nullptr, nullptr)) return; // before the upload
    const size_t out_sz = (size_t)out_rows * out_cols * elem_sz, ov_sz = (size_t)ov_rows * ov_cols * 4;
    Workspace::begin(out_sz + ov_sz + 8192);
    u8 *f = up(frame, out_sz), *o = up(overlay, ov_sz);
    frame_overlay(f, Overlay{1, o, ov_rows, ov_cols, x0, y0, disparity},
                  lens_mode == 0 ? Lens{0, 0.0, 0.0, 0.0} : Lens{lens_mode, pitch, slope, centre},
                  layout == 0 ? Layout{0, 1, 1, 0, 0} : Layout{1, tiles_x, tiles_y, order, 0}, num_views, angle, out_rows, out_cols, elem_sz);
    if (failed()) return; // the caller's frame stays as it was
    down(frame, f, out_sz);
    sync();
}

void stm_d_demux_sbs(unsigned char *d_img_l, unsigned char *d_img_r, unsigned char *d_img_sbs, int num_rows,
                     int num_cols_sbs, int num_cols_out, int elem_sz)
{
    if (!args_ok("d_demux_sbs", {{"num_rows", num_rows, 1}, {"num_cols_sbs", num_cols_sbs, 1},
                                 {"num_cols_out", num_cols_out, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    launch_demux_sbs(d_img_l, d_img_r, d_img_sbs, num_rows, num_cols_sbs, num_cols_out, elem_sz);
}

// NV12 input (an addition, the reference takes BGR only): colour conversion + split as a stage (stm_hip.h)
void stm_d_demux_nv12(unsigned char *d_img_l, unsigned char *d_img_r, unsigned char *d_y, int pitch_y, unsigned char *d_uv, int pitch_uv,
                      int num_rows, int num_cols_sbs, int num_cols_out, int elem_sz, int matrix)
{
    const char *fn = "d_demux_nv12";
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols_sbs", num_cols_sbs, 1}, {"num_cols_out", num_cols_out, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    if (!nv12_args_ok(fn, num_rows, num_cols_sbs, num_cols_out, "num_cols_out", pitch_y, pitch_uv, matrix)) return;
    launch_demux_nv12(d_img_l, d_img_r, d_y, pitch_y, d_uv, pitch_uv, num_rows, num_cols_out, elem_sz, matrix);
}
void stm_demux_nv12(unsigned char *img_l, unsigned char *img_r, unsigned char *y, int pitch_y, unsigned char *uv, int pitch_uv,
                    int num_rows, int num_cols_sbs, int num_cols_out, int elem_sz, int matrix)
{
    const char *fn = "demux_nv12";
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols_sbs", num_cols_sbs, 1}, {"num_cols_out", num_cols_out, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    if (!nv12_args_ok(fn, num_rows, num_cols_sbs, num_cols_out, "num_cols_out", pitch_y, pitch_uv, matrix)) return;
    // a plane's last row need not be a whole pitch long
    const size_t IMG = (size_t)num_rows * num_cols_out * elem_sz, uv_row = 2 * (size_t)((num_cols_sbs + 1) / 2);
    const size_t y_sz = (size_t)(num_rows - 1) * pitch_y + num_cols_sbs, uv_sz = (size_t)(num_rows / 2 - 1) * pitch_uv + uv_row;
    Workspace::begin(2 * IMG + y_sz + uv_sz + 4096);
    u8 *dy = up(y, y_sz), *duv = up(uv, uv_sz), *l = Workspace::get<u8>(IMG), *r = Workspace::get<u8>(IMG);
    if (elem_sz > 3) { // bytes past a pixel's third come back 0, not as the workspace held them
        STM_CHECK(hipMemsetAsync(l, 0, IMG, stream()));
        STM_CHECK(hipMemsetAsync(r, 0, IMG, stream()));
    }
    launch_demux_nv12(l, r, dy, pitch_y, duv, pitch_uv, num_rows, num_cols_out, elem_sz, matrix);
    down(img_l, l, IMG); down(img_r, r, IMG);
    sync();
}

// NV12 output (an addition): the conversion as a stage, the counterpart of stm_demux_nv12 (stm_hip.h)
} // extern "C"
namespace {
bool mux_nv12_args_ok(const char *fn, int pitch_y, int pitch_uv, int num_rows, int num_cols, int elem_sz, int matrix)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 2}, {"num_cols", num_cols, 2}, {"elem_sz", elem_sz, 3}})) return false;
    if (num_rows & 1) return STM_REJECT("num_rows", "%s: num_rows = %d, must be even (a chroma row serves two rows)", fn, num_rows);
    if (num_cols & 1) return STM_REJECT("num_cols", "%s: num_cols = %d, must be even (a chroma sample serves two columns)", fn, num_cols);
    if (pitch_y < num_cols) return STM_REJECT("pitch_y", "%s: pitch_y = %d, must be >= num_cols = %d", fn, pitch_y, num_cols);
    if (pitch_uv < num_cols) return STM_REJECT("pitch_uv", "%s: pitch_uv = %d, must be >= num_cols = %d", fn, pitch_uv, num_cols);
    if (matrix < 0 || matrix > 3)
        return STM_REJECT("matrix", "%s: matrix = %d, must be 0 (BT.601 limited), 1 (BT.709 limited), 2 (BT.601 full) or 3 (BT.709 full)", fn, matrix);
    return true;
}
} // namespace
extern "C" {
void stm_d_mux_nv12(unsigned char *d_y, int pitch_y, unsigned char *d_uv, int pitch_uv, unsigned char *d_img, int num_rows, int num_cols,
                    int elem_sz, int matrix)
{
    if (!mux_nv12_args_ok("d_mux_nv12", pitch_y, pitch_uv, num_rows, num_cols, elem_sz, matrix)) return;
    launch_mux_nv12(nv12_out(d_y, pitch_y, d_uv, pitch_uv, matrix), d_img, num_rows, num_cols, elem_sz);
}
void stm_mux_nv12(unsigned char *y, int pitch_y, unsigned char *uv, int pitch_uv, unsigned char *img, int num_rows, int num_cols, int elem_sz,
                  int matrix)
{
    if (!mux_nv12_args_ok("mux_nv12", pitch_y, pitch_uv, num_rows, num_cols, elem_sz, matrix)) return;
    // a plane's last row need not be a whole pitch long
    const size_t IMG = (size_t)num_rows * num_cols * elem_sz;
    const size_t y_sz = (size_t)(num_rows - 1) * pitch_y + num_cols, uv_sz = (size_t)(num_rows / 2 - 1) * pitch_uv + num_cols;
    Workspace::begin(IMG + y_sz + uv_sz + 4096);
    u8 *di = up(img, IMG), *dy = Workspace::get<u8>(y_sz), *duv = Workspace::get<u8>(uv_sz);
    STM_CHECK(hipMemsetAsync(dy, 0, y_sz, stream())); // the bytes between a row's samples and the next row come back 0
    STM_CHECK(hipMemsetAsync(duv, 0, uv_sz, stream()));
    launch_mux_nv12(nv12_out(dy, pitch_y, duv, pitch_uv, matrix), di, num_rows, num_cols, elem_sz);
    down(y, dy, y_sz); down(uv, duv, uv_sz);
    sync();
}


// packed input (an addition): the unpacking as a stage, from a BGR frame and from NV12 planes (stm_hip.h)
void stm_d_demux_packed(unsigned char *d_img_l, unsigned char *d_img_r, unsigned char *d_img, int num_rows, int num_cols_sbs,
                        int num_cols_out, int elem_sz, int packing, int swap, int filter, int gap)
{
    const char *fn = "d_demux_packed";
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols_sbs", num_cols_sbs, 1}, {"num_cols_out", num_cols_out, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    const Packing pk = {packing, swap, filter, gap};
    if (!packing_args_ok(fn, pk, num_rows, num_cols_sbs, num_cols_out, "num_cols_out", false, 0, 0, 0)) return;
    launch_demux_packed(d_img_l, d_img_r, PackInput{pk, false, d_img, num_cols_sbs, nullptr, nullptr, 0, 0, 0}, num_rows, num_cols_out, elem_sz);
}
void stm_demux_packed(unsigned char *img_l, unsigned char *img_r, unsigned char *img, int num_rows, int num_cols_sbs, int num_cols_out,
                      int elem_sz, int packing, int swap, int filter, int gap)
{
    const char *fn = "demux_packed";
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols_sbs", num_cols_sbs, 1}, {"num_cols_out", num_cols_out, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    const Packing pk = {packing, swap, filter, gap};
    if (!packing_args_ok(fn, pk, num_rows, num_cols_sbs, num_cols_out, "num_cols_out", false, 0, 0, 0)) return;
    const size_t IMG = (size_t)num_rows * num_cols_out * elem_sz, in_sz = (size_t)pk.rows_f(num_rows) * num_cols_sbs * elem_sz;
    Workspace::begin(2 * IMG + in_sz + 4096);
    u8 *d = up(img, in_sz), *l = Workspace::get<u8>(IMG), *r = Workspace::get<u8>(IMG);
    if (elem_sz > 3) { // bytes past a pixel's third come back 0, not as the workspace held them
        STM_CHECK(hipMemsetAsync(l, 0, IMG, stream()));
        STM_CHECK(hipMemsetAsync(r, 0, IMG, stream()));
    }
    launch_demux_packed(l, r, PackInput{pk, false, d, num_cols_sbs, nullptr, nullptr, 0, 0, 0}, num_rows, num_cols_out, elem_sz);
    down(img_l, l, IMG); down(img_r, r, IMG);
    sync();
}
void stm_d_demux_nv12_packed(unsigned char *d_img_l, unsigned char *d_img_r, unsigned char *d_y, int pitch_y, unsigned char *d_uv,
                             int pitch_uv, int num_rows, int num_cols_sbs, int num_cols_out, int elem_sz, int matrix, int packing, int swap,
                             int filter, int gap)
{
    const char *fn = "d_demux_nv12_packed";
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols_sbs", num_cols_sbs, 1}, {"num_cols_out", num_cols_out, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    const Packing pk = {packing, swap, filter, gap};
    if (!packing_args_ok(fn, pk, num_rows, num_cols_sbs, num_cols_out, "num_cols_out", true, pitch_y, pitch_uv, matrix)) return;
    launch_demux_packed(d_img_l, d_img_r, PackInput{pk, true, nullptr, num_cols_sbs, d_y, d_uv, pitch_y, pitch_uv, matrix}, num_rows,
                        num_cols_out, elem_sz);
}
void stm_demux_nv12_packed(unsigned char *img_l, unsigned char *img_r, unsigned char *y, int pitch_y, unsigned char *uv, int pitch_uv,
                           int num_rows, int num_cols_sbs, int num_cols_out, int elem_sz, int matrix, int packing, int swap, int filter,
                           int gap)
{
    const char *fn = "demux_nv12_packed";
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols_sbs", num_cols_sbs, 1}, {"num_cols_out", num_cols_out, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    const Packing pk = {packing, swap, filter, gap};
    if (!packing_args_ok(fn, pk, num_rows, num_cols_sbs, num_cols_out, "num_cols_out", true, pitch_y, pitch_uv, matrix)) return;
    // the planes follow the frame's rows; a plane's last row need not be a whole pitch long
    const int rows_f = pk.rows_f(num_rows);
    const size_t IMG = (size_t)num_rows * num_cols_out * elem_sz, uv_row = 2 * (size_t)((num_cols_sbs + 1) / 2);
    const size_t y_sz = (size_t)(rows_f - 1) * pitch_y + num_cols_sbs, uv_sz = (size_t)(rows_f / 2 - 1) * pitch_uv + uv_row;
    Workspace::begin(2 * IMG + y_sz + uv_sz + 4096);
    u8 *dy = up(y, y_sz), *duv = up(uv, uv_sz), *l = Workspace::get<u8>(IMG), *r = Workspace::get<u8>(IMG);
    if (elem_sz > 3) {
        STM_CHECK(hipMemsetAsync(l, 0, IMG, stream()));
        STM_CHECK(hipMemsetAsync(r, 0, IMG, stream()));
    }
    launch_demux_packed(l, r, PackInput{pk, true, nullptr, num_cols_sbs, dy, duv, pitch_y, pitch_uv, matrix}, num_rows, num_cols_out, elem_sz);
    down(img_l, l, IMG); down(img_r, r, IMG);
    sync();
}

} // extern "C"

// device staging buffers of the blocking host-flavour frame calls: grow-only, one set per host thread and device (the
// reference's adcensus_stm allocates and frees them on every frame, d_io.cu:43-235)
namespace {
struct HostFrameBufs {
    void *p[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t cap[4] = {0, 0, 0, 0};
};
constexpr int HFB_DEVS = 64;
thread_local HostFrameBufs g_hfb[HFB_DEVS];
// returns false (error recorded, nothing usable) if an allocation fails
bool host_frame_bufs(const size_t (&bytes)[4], void *(&out)[4])
{
    const int dev = cur_dev();
    if (dev < 0 || dev >= HFB_DEVS) {
        fail("adcensus_stm: device index out of range", "cur_dev", __FILE__, __LINE__);
        return false;
    }
    HostFrameBufs &b = g_hfb[dev];
    for (int i = 0; i < 4; ++i) {
        if (bytes[i] > b.cap[i]) {
            if (b.p[i]) {
                STM_CHECK(hipStreamSynchronize(stream()));
                STM_CHECK(hipFree(b.p[i]));
                b.p[i] = nullptr;
                b.cap[i] = 0;
            }
            void *q = nullptr;
            if (hipMalloc(&q, bytes[i]) != hipSuccess || !q) {
                (void)hipGetLastError();
                fail("adcensus_stm: device buffer allocation failed", "hipMalloc", __FILE__, __LINE__);
                return false;
            }
            b.p[i] = q;
            b.cap[i] = bytes[i];
        }
        out[i] = b.p[i];
    }
    return true;
}
} // namespace

// stm_release_workspace(): a thread that ends frees these together with its workspace
namespace stm {
void release_host_frame_bufs()
{
    int keep = 0;
    if (hipGetDevice(&keep) != hipSuccess) return;
    for (int dev = 0; dev < HFB_DEVS; ++dev) {
        HostFrameBufs &b = g_hfb[dev];
        bool any = false;
        for (int i = 0; i < 4; ++i) any = any || b.p[i];
        if (!any) continue;
        STM_CHECK(hipSetDevice(dev));
        STM_CHECK(hipDeviceSynchronize());
        for (int i = 0; i < 4; ++i) {
            if (b.p[i]) STM_CHECK(hipFree(b.p[i]));
            b.p[i] = nullptr;
            b.cap[i] = 0;
        }
    }
    STM_CHECK(hipSetDevice(keep));
}
} // namespace stm

// =============================================================== whole frame
// adcensus_stm, d_io.cu:7-238: demux -> cost init -> aggregation (L, R) -> WTA -> DCC -> IRV x5 ->
// bilateral(7,5,10) -> hit maps -> bleed(1) -> masks -> N-2 synthesised views -> interlace.
// Differences in mechanics (not in results): one cached workspace instead of ~35 cudaMalloc/cudaFree,
// no host synchronisation inside the frame, quad-interleaved volumes, the last aggregation pass is fused
// with WTA, both views share the arms / IRV launches, the mask blur G(1 - maskR) is computed once per frame
// instead of once per view (it does not depend on the view).
namespace {

// A frame call's arguments: the reference's, in its order (num_rows .. thresh_h), the `stages` word (3 where the entry has none;
// bit 0x2000 is the entry's business -- no body looks at it) and the match size of the reduced-resolution calls.  Each extern "C"
// frame entry fills one and the screens, the bodies and the host flavour take it by reference.
struct FrameArgs {
    int num_rows, num_cols_sbs, num_cols, num_rows_out, num_cols_out, elem_sz, num_views;
    float angle;
    int num_disp, zero_disp;
    float ad_coeff, census_coeff, ucd, lcd;
    int usd, lsd, thresh_s;
    float thresh_h;
    int stages;
    int num_rows_disp = 0, num_cols_disp = 0; // the reduced-resolution calls only
    float disp_scale = 0.0f;
};

// cost init .. WTA (.. DCC/IRV/bilateral when `refine`) on one rectified pair H x W already split into L / R, with a's matching
// parameters and a's `stages` bits 0x100 (HSLO), 0x200 (sub-pixel) and 0x400 (outlier interpolation)
// pre: optional {BGRX left, BGRX right, wide left, wide right, census left, census right} planes produced together with the split
// (full-resolution path); the census pair may be null (then it is computed here)
void frame_disparity(u8 *img_l, u8 *img_r, float *d_disp_l, float *d_disp_r, int H, int W, const FrameArgs &a, bool refine,
                     uint32_t *const *pre)
{
    const int elem_sz = a.elem_sz, D = a.num_disp, zero_disp = a.zero_disp, usd = a.usd, lsd = a.lsd, thresh_s = a.thresh_s;
    const float ad_coeff = a.ad_coeff, census_coeff = a.census_coeff, ucd = a.ucd, lcd = a.lcd, thresh_h = a.thresh_h;
    const bool hslo = stages_hslo(a.stages), subpix = stages_subpix(a.stages);
    const bool interp = (a.stages & 0x400) != 0; // + interpolation of the outliers region voting leaves (Mei et al. 3.4)
    const size_t HW = (size_t)H * W;
    const int NQ = (D + 3) / 4;
    const size_t V = HW * NQ * 4; // volumes are kept quad-interleaved (float4 [NQ][H][W]) inside the frame
    const bool matrix_pipe = agg_on_matrix_pipe(usd, H, W); // default aggregation path: stm_kernels_aggm.hip
    float *cost = matrix_pipe ? nullptr : Workspace::get<float>(2 * V), *scratch = matrix_pipe ? nullptr : Workspace::get<float>(V);
    uint32_t *pk_l = pre ? pre[0] : Workspace::get<uint32_t>(HW), *pk_r = pre ? pre[1] : Workspace::get<uint32_t>(HW);
    Vol cl = vol_quads(cost, HW), cr = vol_quads(cost ? cost + V : nullptr, HW), sc = vol_quads(scratch, HW);
    // the first aggregation pass computes the initial costs itself (COST mode) and the 2 V of initial costs are never
    // written; only HSLO on the vector-ALU path and the per-stage API materialise them with stm_k_cost_init
    const bool cost_volume = hslo && !matrix_pipe;
    uint32_t *cen[2] = {nullptr, nullptr};
    core_ci(img_l, img_r, cl, cr, pk_l, pk_r, ad_coeff, census_coeff, D, zero_disp, H, W, elem_sz, pre != nullptr,
            cost_volume ? nullptr : cen, pre && pre[4] ? pre + 4 : nullptr);

    const Arms al = carve_arms(HW), ar = carve_arms(HW);
    uint32_t *htab = nullptr, *vtab = nullptr;
    int vrec = 0, vtop = -1;
    bool vcol = false;
    {
        const uint32_t *pk[2] = {pk_l, pk_r};
        u8 *u[2] = {al.up, ar.up}, *d[2] = {al.down, ar.down}, *l[2] = {al.left, ar.left}, *r[2] = {al.right, ar.right};
        const uint32_t *wide[2] = {pre ? pre[2] : nullptr, pre ? pre[3] : nullptr};
        // the last aggregation pass's horizontal window table comes out of the same kernel (it has the arms in registers)
        const size_t hw_dw = matrix_pipe ? aggm_frame_htab_dwords(D, H, W, usd, hslo) : 0;
        htab = hw_dw ? Workspace::get<uint32_t>(hw_dw) : nullptr;
        // (both tables or the horizontal one alone; with sub-pixel enhancement the last pass's input is read again as a PQ volume)
        const size_t vw_dw = matrix_pipe && htab ? aggm_frame_vtab_dwords(D, zero_disp, H, W, usd, hslo, subpix, &vrec, &vtop, &vcol) : 0;
        vtab = vw_dw ? Workspace::get<uint32_t>(vw_dw) : nullptr;
        launch_cross_arms2(2, pk, u, d, l, r, ucd, lcd, usd, lsd, H, W, pre ? wide : nullptr, htab, vtab, vrec, vtop, vcol);
    }
    // with refinement the raw WTA maps live in scratch and the bilateral filter, the last step, writes the caller's buffers
    float *wl = refine ? Workspace::get<float>(HW) : d_disp_l, *wr = refine ? Workspace::get<float>(HW) : d_disp_r;
    // HSLO = Mei et al. 3.3: scanline optimisation of the aggregated cost, then WTA.  Penalty constants: the values the
    // reference's (commented-out) test call uses, image_io.cpp:311-313.  Parity unpinned.
    const u8 *hs_a[2] = {img_l, img_r}, *hs_b[2] = {img_r, img_l}; // the right view's own image plays "left"
    const int hs_sign[2] = {1, -1};
    float *v2_pq[2] = {nullptr, nullptr}, *v2_quads[2] = {nullptr, nullptr}; // the input of the last horizontal pass, per view
    if (matrix_pipe) {
        // the aggregation kernels on the matrix pipe: cost -> H -> V, V -> H (+ WTA, or + the HSLO passes on the volume), two
        // PQ-layout volumes per view
        const size_t VP = pq_volume_floats(D, H, W);
        float *m = Workspace::get<float>(4 * VP);
        float *va[2] = {m, m + VP}, *vb[2] = {m + 2 * VP, m + 3 * VP};
        const uint32_t *pk[2] = {pk_l, pk_r}, *cn[2] = {cen[0], cen[1]};
        const u8 *u[2] = {al.up, ar.up}, *d[2] = {al.down, ar.down}, *l[2] = {al.left, ar.left}, *r[2] = {al.right, ar.right};
        float *dv[2] = {wl, wr};
        launch_aggm_frame(pk, cn, rho_table(ad_coeff, census_coeff), va, vb, u, d, l, r, dv, D, zero_disp, H, W, usd, hslo, htab, vtab, subpix);
        if (hslo) launch_hslo_wta_pq(2, vb, va, hs_a, hs_b, hs_sign, dv, 15.0f, 1.0f, 3.0f, D, zero_disp, H, W, elem_sz);
        v2_pq[0] = va[0]; // the last horizontal pass's input (written by the vertical passes, read by the pass + WTA, kept)
        v2_pq[1] = va[1];
    } else if (hslo) {
        core_agg(cl, sc, al, D, H, W, usd);
        core_agg(cr, sc, ar, D, H, W, usd);
        const Vol cv[2] = {cl, cr};
        float *dv[2] = {wl, wr};
        launch_hslo_wta(2, cv, hs_a, hs_b, hs_sign, dv, 15.0f, 1.0f, 3.0f, D, zero_disp, H, W, elem_sz);
    } else {
        // legacy (stm_set_agg_variant(10000)): H, V, V per view on the vector ALU, then the last H pass + WTA of both views in one launch.  After three passes a view's
        // data sits in its scratch volume; the right view uses the left view's (now free) cost volume as scratch.
        float *scratch2 = Workspace::get<float>(V);
        Vol s2 = vol_quads(scratch2, HW);
        launch_agg_h2_cost(pk_l, cen[0], pk_r, cen[1], rho_table(ad_coeff, census_coeff), sc, al.left, al.right, s2, ar.left, ar.right,
                           D, zero_disp, H, W);
        const AggTap tap = agg_tap(); // the test tap (stm_set_agg_tap): copies behind the passes, no h4 (this chain keeps no last volume)
        if (tap.h1) launch_tap_read(sc.base, s2.base, TAP_QUADS, 0, tap.h1, D, H, W);
        launch_agg_v(sc, cl, al.up, al.down, D, H, W, usd);
        launch_agg_v(s2, cr, ar.up, ar.down, D, H, W, usd);
        launch_agg_v(cl, sc, al.up, al.down, D, H, W, usd);
        launch_agg_v(cr, s2, ar.up, ar.down, D, H, W, usd);
        if (tap.v2) launch_tap_read(sc.base, s2.base, TAP_QUADS, 0, tap.v2, D, H, W);
        if (tap.inject_v2) launch_tap_write(sc.base, s2.base, TAP_QUADS, 0, tap.inject_v2, D, H, W);
        launch_agg_h_wta2(sc, al.left, al.right, wl, s2, ar.left, ar.right, wr, D, zero_disp, H, W);
        v2_quads[0] = sc.base;
        v2_quads[1] = s2.base;
    }
    // sub-pixel enhancement (0x200): the parabola through the costs at d - 1, d, d + 1, rebuilt from the last horizontal pass's
    // input, which nothing below overwrites (DCC / IRV carve their own workspace).  Without refinement it runs on the WTA maps
    // here; with it, after region voting (DCC and IRV keep working on whole numbers) and before the bilateral filter.
    float *sp_dv[2] = {wl, wr};
    const u8 *sp_l[2] = {al.left, ar.left}, *sp_r[2] = {al.right, ar.right};
    if (!refine) {
        if (subpix) launch_subpix_frame(v2_pq[0] ? v2_pq : nullptr, v2_quads, sp_dv, sp_l, sp_r, D, zero_disp, H, W);
        return;
    }

    u8 *outl_l = Workspace::get<u8>(HW), *outl_r = Workspace::get<u8>(HW);
    {   // d_io.cu:138-143 (outlier maps zeroed, dr_dcc) and :147-148, both views per launch
        float *dv[2] = {wl, wr};
        u8 *ov[2] = {outl_l, outl_r};
        const u8 *u[2] = {al.up, ar.up}, *d[2] = {al.down, ar.down}, *l[2] = {al.left, ar.left}, *r[2] = {al.right, ar.right};
        launch_irv(2, dv, ov, u, d, l, r, thresh_s, thresh_h, H, W, D, zero_disp, usd, 5, true, true);
    }
    // outlier interpolation (0x400): what region voting left marked takes a reliable neighbour's value, each view on its own image
    // and its own post-voting outlier map (the vote kernels clear a pixel's mark when they accept it).  The values written are
    // copies of values in the map, so the maps stay whole-number and in range for the sub-pixel step and the bilateral filter.
    if (interp) {
        const u8 *ov[2] = {outl_l, outl_r}, *iv[2] = {img_l, img_r};
        launch_interp(2, sp_dv, ov, iv, H, W, elem_sz);
    }
    if (subpix) launch_subpix_frame(v2_pq[0] ? v2_pq : nullptr, v2_quads, sp_dv, sp_l, sp_r, D, zero_disp, H, W);
    // the maps are this pipeline's own WTA / region-voting output: integer-valued, any two of them differ by at most D - 1 --
    // unless the sub-pixel step has run: then almost no tile is integer-valued and the general form is taken directly
    launch_bilateral2(wl, d_disp_l, wr, d_disp_r, gauss2d_table(7, 10.0f), gauss1d_table(D, 5.0f), 7, H, W, D, !subpix, // :150-151  (7, 5, 10)
                      bilateral_one_value_table(D, zero_disp, 10.0f, 5.0f), zero_disp);
}

// the thread's output format (stm_set_output) against a rendering frame call's geometry under the already screened layout `lo`
static bool frame_output_ok(const char *fn, const Layout &lo, int Hout, int Wout)
{
    const Output o = output();
    if (o.format == 0) return true;
    const long long P = o.pitch ? o.pitch : Wout, R = o.uv_row ? o.uv_row : Hout;
    if (lo.layout == 0)
        return STM_REJECT("format, layout", "%s: output format 1 (NV12) exists for quilts only (chroma subsampling destroys a sub-pixel interlaced "
                          "frame): set a layout (stm_set_layout) or format 0", fn);
    if (Hout & 1) return STM_REJECT("num_rows_out", "%s: num_rows_out = %d, must be even for NV12 output (a chroma row serves two rows)", fn, Hout);
    if (Wout & 1)
        return STM_REJECT("num_cols_out", "%s: num_cols_out = %d, must be even for NV12 output (a chroma sample serves two columns)", fn, Wout);
    if ((Wout / lo.tiles_x) & 1)
        return STM_REJECT("num_cols_out", "%s: tile width num_cols_out / tiles_x = %d, must be even for NV12 output (every tile starts on a chroma "
                          "sample)", fn, Wout / lo.tiles_x);
    if ((Hout / lo.tiles_y) & 1)
        return STM_REJECT("num_rows_out", "%s: tile height num_rows_out / tiles_y = %d, must be even for NV12 output (every tile starts on a chroma "
                          "sample)", fn, Hout / lo.tiles_y);
    if (P < Wout) return STM_REJECT("pitch", "%s: the NV12 surface's pitch = %lld, must be >= num_cols_out = %d", fn, P, Wout);
    if (R < Hout) return STM_REJECT("uv_row", "%s: the NV12 surface's uv_row = %lld, must be >= num_rows_out = %d", fn, R, Hout);
    return true; // pitch * (uv_row + num_rows_out / 2) < 2^31 * 1.5 * 2^31 < 2^63 for every int
}
// the thread's layout (stm_set_layout) against a rendering frame call's geometry, before anything is launched; layout 0, or a call
// that renders nothing: nothing to check, the call is as it was.  The thread's output format (stm_set_output) is screened here too.
bool frame_layout_ok(const char *fn, const FrameArgs &a)
{
    const Layout lo = layout();
    const int num_views = a.num_views, Hout = a.num_rows_out, Wout = a.num_cols_out;
    if ((a.stages & 0xff) < 3) return true;
    if (overlay().mode == 1) { // an overlay (stm_set_overlay) is composited on BGR frames only
        if (output().format == 1)
            return STM_REJECT("overlay, format", "%s: an overlay (stm_set_overlay) together with output format 1 (NV12): compositing on a "
                              "chroma-subsampled surface is not defined, set one of them to 0", fn);
        if (!overlay_tiles_ok(fn, lo, num_views)) return false;
        if (overlay_auto().mode == 1 && !overlay_fit_size_ok(fn, a.num_rows, a.num_cols)) return false;
    }
    if (lo.layout == 0) return frame_output_ok(fn, lo, Hout, Wout);
    if (lens().mode != 0)
        return STM_REJECT("layout, lens", "%s: layout 1 (quilt) together with lens mode %d: a quilt is not interlaced, set one of them to 0", fn,
                          lens().mode);
    return quilt_args_ok(fn, lo, num_views, a.num_rows, a.num_cols, Hout, Wout, "num_views", "num_rows_out", "num_cols_out") &&
           frame_output_ok(fn, lo, Hout, Wout);
}

// hit maps -> bleed -> masks -> N-2 views -> interlace (d_io.cu:160-205)
// depth_state_out: where depth mode 2's state lies, the workspace's four floats included (null in the other modes)
// d_rect: the active rectangle mode 2's fit is restricted to (stm_set_active), or null
void frame_render(u8 *img_l, u8 *img_r, float *d_disp_l, float *d_disp_r, u8 *d_interlaced, const FrameArgs &a, float **depth_state_out,
                  const int *d_rect)
{
    *depth_state_out = nullptr;
    const int H = a.num_rows, W = a.num_cols, Hout = a.num_rows_out, Wout = a.num_cols_out, elem_sz = a.elem_sz, N = a.num_views;
    const float angle = a.angle;
    const bool linear = (a.stages & 0x800) != 0; // the views' warps fetched at the fractional coordinate (stm_dibr_dbm_lin)
    const size_t HW = (size_t)H * W, IMG = HW * elem_sz;
    float *mask_l = Workspace::get<float>(HW), *mask_r = Workspace::get<float>(HW), *blend = Workspace::get<float>(HW);
    launch_hitmask_rows(mask_l, mask_r, d_disp_l, d_disp_r, H, W); // :165-176: dibr_occl, bleed(1) x2, occl_to_mask
    launch_gaussian_max(mask_r, blend, gauss2d_table(10, 15.0f), 10, 15.0f, H, W, true); // d_dibr_bwarp.cu:60-63, once per frame

    // a lens geometry (stm_set_lens) replaces the reference's view assignment; `angle` is then neither used nor screened.  Mode 3
    // renders every sub-pixel at a position of its own -- there are no views to write -- so it takes the fused kernel always
    const Lens ln = lens();
    // a depth budget (stm_set_depth) maps every view's position to the shift it is rendered at and to an offset of its sampling
    // position: as in lens mode 3 there are no views to write, so the fused kernel is taken always.  Mode 2 first measures the maps
    // this render reads (the up-scaled ones of the reduced frame, the stabilised ones of 0x2000) and leaves gain and conv in the
    // state, which the renderer reads on the device.
    const Depth dp = depth();
    // a quilt (stm_set_layout) replaces the interlacer altogether: the views are tiled, whole.  The caller has screened the tiling
    // (frame_layout_ok).  With a depth budget there are no views to write; without one, 200 writes every view and tiles the table.
    // Under stm_set_output's format 1 d_interlaced is an NV12 surface (screened by frame_layout_ok) and the quilt's kernels convert the
    // pixels they render; 200 with depth mode 0 writes the BGR quilt into the workspace and converts that (stm_k_mux_nv12).
    const Layout lo = layout();
    // the reference's view assignment from `angle`, which the depth renderer of the interlaced frame takes: screened before the fit
    float inv_y = 0.0f;
    int ymod = 1;
    if (lo.layout == 0 && dp.mode != 0 && ln.mode == 0 && !mux_geom_ok(N, angle, elem_sz, nullptr, &inv_y, &ymod)) return;
    // mode 2's fit, ahead of everything that reads gain and conv from the state: the prefilter below and the renderer
    float *state = nullptr;
    if (dp.mode == 2) {
        uint32_t *hist = Workspace::get<uint32_t>(4096);
        state = dp.d_state ? dp.d_state : Workspace::get<float>(4);
        launch_depth_fit(state, hist, d_disp_l, d_disp_r, H, W, dp.disp_lo, dp.disp_hi, dp.max_gain, dp.clip_permille, dp.rate,
                         dp.d_state == nullptr, d_rect);
        *depth_state_out = state;
    }
    // view antialiasing (stm_set_antialias): both images filtered by their own maps into fresh workspace, and every renderer below
    // takes the filtered pair -- the caller's images (0x2000's history, _nv12's outputs) and the maps stay as they are.  The displayed
    // disparity of a pixel is gain * delta - conv under a depth budget, delta itself without one
    const Antialias aa = antialias();
    if (aa.mode == 1) {
        u8 *flt[2] = {Workspace::get<u8>(IMG), Workspace::get<u8>(IMG)};
        const u8 *src[2] = {img_l, img_r};
        const float *dsp[2] = {d_disp_l, d_disp_r};
        launch_view_prefilter(2, flt, src, dsp, H, W, elem_sz, N, aa.strength, aa.max_radius, aa.gate, dp.mode == 1 ? dp.gain : 1.0f,
                              dp.mode == 1 ? dp.conv : 0.0f, state);
        img_l = flt[0];
        img_r = flt[1];
    }
    if (lo.layout == 1) {
        const Output of = output();
        const Nv12Out surf = of.format == 1 ? nv12_out_surface(d_interlaced, of, Hout, Wout) : Nv12Out{};
        const Nv12Out *nv = of.format == 1 ? &surf : nullptr;
        if (dp.mode == 0 && (agg_variant() / 100) % 10 == 2) {
            u8 *views_mem = Workspace::get<u8>((size_t)N * IMG);
            launch_view_synth_all(views_mem, IMG, N, img_l, img_r, d_disp_l, d_disp_r, mask_l, mask_r, blend, H, W, elem_sz, linear);
            u8 **dv = Workspace::get<u8 *>(N);
            launch_view_table(dv, img_r, img_l, views_mem, IMG, N);
            u8 *quilt = nv ? Workspace::get<u8>((size_t)Hout * Wout * elem_sz) : d_interlaced;
            launch_quilt((const u8 *const *)dv, quilt, N, lo, H, W, Hout, Wout, elem_sz);
            if (nv) launch_mux_nv12(surf, quilt, Hout, Wout, elem_sz);
            return;
        }
        launch_synth_quilt(img_l, img_r, d_disp_l, d_disp_r, mask_l, mask_r, blend, d_interlaced, N, lo, dp.mode, dp.gain, dp.conv, state, H, W,
                           Hout, Wout, elem_sz, linear, nv);
        return;
    }
    if (dp.mode != 0) {
        launch_synth_mux_depth(img_l, img_r, d_disp_l, d_disp_r, mask_l, mask_r, blend, d_interlaced, N, ln, inv_y, ymod, dp.gain, dp.conv,
                               state, H, W, Hout, Wout, elem_sz, linear);
        return;
    }
    if (ln.mode != 0 && (ln.mode == 3 || (agg_variant() / 100) % 10 != 2)) {
        launch_synth_mux_lens(img_l, img_r, d_disp_l, d_disp_r, mask_l, mask_r, blend, d_interlaced, N, ln, H, W, Hout, Wout, elem_sz, linear);
        return;
    }
    if (ln.mode != 0) { // 200: every view written, then interlaced through the lens
        u8 *views_mem = Workspace::get<u8>((size_t)N * IMG);
        launch_view_synth_all(views_mem, IMG, N, img_l, img_r, d_disp_l, d_disp_r, mask_l, mask_r, blend, H, W, elem_sz, linear);
        u8 **dv = Workspace::get<u8 *>(N);
        launch_view_table(dv, img_r, img_l, views_mem, IMG, N);
        launch_mux_lens((const u8 *const *)dv, d_interlaced, N, ln, H, W, Hout, Wout, elem_sz);
        return;
    }
    if ((agg_variant() / 100) % 10 != 2) {
        // views + interlacing in one pass: an output pixel synthesises exactly the samples it interlaces (stm_k_synth_mux)
        float yi, inv_y;
        int ymod;
        if (!mux_geom_ok(N, angle, elem_sz, &yi, &inv_y, &ymod)) return;
        launch_synth_mux(img_l, img_r, d_disp_l, d_disp_r, mask_l, mask_r, blend, d_interlaced, N, yi, inv_y, ymod, H, W, Hout, Wout, elem_sz, 2,
                         linear);
        return;
    }
    // 200: the un-fused form (every view written, then interlaced), as the reference structures it (d_io.cu:182-203)
    u8 *views_mem = Workspace::get<u8>((size_t)N * IMG);
    // views[0] = right image, views[N-1] = left image (d_io.cu:182-183)
    launch_view_synth_all(views_mem, IMG, N, img_l, img_r, d_disp_l, d_disp_r, mask_l, mask_r, blend, H, W, elem_sz, linear); // :186-201
    // view table built on the device (no host memory involved, so nothing to keep alive or synchronise)
    u8 **dv = Workspace::get<u8 *>(N);
    launch_view_table(dv, img_r, img_l, views_mem, IMG, N);
    core_mux((const u8 *const *)dv, d_interlaced, N, angle, H, W, Hout, Wout, elem_sz, 2); // :203
}

// the history of the temporal stabilisation (stages bit 0x2000, stm_d_adcensus_stm_t): the previous frame's side-by-side input and
// the two maps it put out
struct TemporalHist {
    const u8 *sbs; // stm_d_adcensus_stm_t: read in place, each view in its own half
    const float *disp_l, *disp_r;
    float alpha;
    int thresh_color;
    float thresh_disp;
    const u8 *img_l = nullptr, *img_r = nullptr; // stm_d_adcensus_stm_nv12: the previous frame's converted split images
};
// the input of stm_d_adcensus_stm_nv12 in place of d_img_sbs: the two planes, and where the converted split images go (both null:
// the workspace)
struct Nv12Input {
    const u8 *y, *uv;
    int pitch_y, pitch_uv, matrix;
    u8 *img_l, *img_r;
};

// ---- the vertical alignment of a frame call's input (stm_set_align)
// the thread's setting against a frame call's geometry; off: nothing to check, the call is as it was
bool frame_align_ok(const char *fn, int num_rows, int num_cols_sbs, int num_cols, bool bgr_sbs)
{
    const Align al = align();
    if (!al.mode) return true;
    if (bgr_sbs && num_cols_sbs < 2 * num_cols) // both eyes are gathered from the frame
        return STM_REJECT("num_cols_sbs", "%s: an alignment is set on this thread (stm_set_align), which needs num_cols_sbs >= 2 * num_cols", fn);
    return al.mode != 2 || align_size_ok(fn, num_rows, num_cols);
}
// the workspace the prelude below takes: the aligned frame (and the previous frame's), the profiles, the SADs, a scratch state
size_t align_ws_bytes(int H, size_t IMG, bool prev) { return (prev ? 4 : 2) * IMG + (align_profile_words(H) + align_sad_words(32)) * 4 + 4096; }
// The prelude, inside the frame call's Workspace scope: mode 2 measures the screened frame `in` at full resolution and updates the
// state; the aligned, unpacked, converted pair is returned as one side-by-side BGR frame (H x 2 W x elem_sz) in the workspace.
// prev_frame != nullptr: the previous BGR frame, of the same geometry, through the same kernel with THIS frame's field into prev_out.
u8 *align_frame_input(const Align &al, const PackInput &in, const u8 *prev_frame, int H, int W, int elem_sz, const u8 *&prev_out)
{
    const size_t IMG = (size_t)H * W * elem_sz;
    const float *st = nullptr;
    if (al.mode == 2) {
        float *state = al.d_state ? al.d_state : Workspace::get<float>(4); // scratch: every frame on its own
        uint32_t *prof = Workspace::get<uint32_t>(align_profile_words(H)), *sad = Workspace::get<uint32_t>(align_sad_words(al.radius));
        launch_align_measure(state, nullptr, prof, sad, &in, nullptr, nullptr, H, W, elem_sz, al.radius, al.rate, al.d_state == nullptr);
        st = state;
    }
    u8 *out = Workspace::get<u8>(2 * IMG);
    launch_align_frame(out, &in, nullptr, H, W, elem_sz, al.a, al.b, al.c, st);
    prev_out = nullptr;
    if (prev_frame) {
        PackInput prev = in;
        prev.frame = prev_frame;
        u8 *po = Workspace::get<u8>(2 * IMG);
        launch_align_frame(po, &prev, nullptr, H, W, elem_sz, al.a, al.b, al.c, st);
        prev_out = po;
    }
    return out;
}

// ---- the rectification of a frame call's input (a frame stream's stm_stream_rectify), ahead of every other prelude
// the thread's setting against a frame call's geometry; off: nothing to check, the call is as it was
bool frame_rectify_ok(const char *fn, int num_cols_sbs, int num_cols, bool bgr_sbs)
{
    if (!rectify().mode) return true;
    if (bgr_sbs && num_cols_sbs < 2 * num_cols) // both eyes are gathered from the frame
        return STM_REJECT("num_cols_sbs", "%s: a rectification is on (stm_stream_rectify), which needs num_cols_sbs >= 2 * num_cols", fn);
    return true;
}
// the workspace the prelude below takes: the rectified frame (and the previous frame's)
size_t rectify_ws_bytes(size_t IMG, bool prev) { return (prev ? 4 : 2) * IMG + 1024; }
// The prelude, inside the frame call's Workspace scope: the unpacked, converted pair, each eye through its record, returned as one
// side-by-side BGR frame (H x 2 W x elem_sz) in the workspace.  prev_frame != nullptr: the previous BGR frame, of the same
// geometry, through the same kernel with the same records into prev_out.
u8 *rectify_frame_input(const Rectify &rc, const PackInput &in, const u8 *prev_frame, int H, int W, int elem_sz, const u8 *&prev_out)
{
    const size_t IMG = (size_t)H * W * elem_sz;
    u8 *out = Workspace::get<u8>(2 * IMG);
    launch_rectify_frame(out, &in, nullptr, H, W, elem_sz, rc.rec, rc.border);
    prev_out = nullptr;
    if (prev_frame) {
        PackInput prev = in;
        prev.frame = prev_frame;
        u8 *po = Workspace::get<u8>(2 * IMG);
        launch_rectify_frame(po, &prev, nullptr, H, W, elem_sz, rc.rec, rc.border);
        prev_out = po;
    }
    return out;
}

// ---- the colour balance of a frame call's input (stm_set_balance), after the alignment
// the thread's setting against a frame call's geometry; off: nothing to check, the call is as it was
bool frame_balance_ok(const char *fn, int num_rows, int num_cols_sbs, int num_cols, bool bgr_sbs)
{
    const Balance bl = balance();
    if (!bl.mode) return true;
    if (bgr_sbs && num_cols_sbs < 2 * num_cols) // both eyes are gathered from the frame
        return STM_REJECT("num_cols_sbs", "%s: a colour balance is set on this thread (stm_set_balance), which needs num_cols_sbs >= 2 * num_cols", fn);
    return bl.mode != 2 || balance_size_ok(fn, num_rows, num_cols);
}
// the workspace the prelude below takes: the balanced frame (and the previous frame's), the histograms, a scratch state
size_t balance_ws_bytes(size_t IMG, bool prev) { return (prev ? 4 : 2) * IMG + (BALANCE_HIST_WORDS + BALANCE_STATE_WORDS) * 4 + 4096; }
// The prelude, inside the frame call's Workspace scope, after the alignment's: mode 2 measures the screened frame `in` (the aligned
// frame where an alignment is on) and updates the state; the unpacked, converted pair, its right eye through the tables, is returned
// as one side-by-side BGR frame (H x 2 W x elem_sz) in the workspace.  prev_frame != nullptr: the previous BGR frame, of the same
// geometry, through the same kernel with THIS frame's tables into prev_out.
u8 *balance_frame_input(const Balance &bl, const PackInput &in, const u8 *prev_frame, int H, int W, int elem_sz, const u8 *&prev_out)
{
    const size_t IMG = (size_t)H * W * elem_sz;
    const int *st = nullptr;
    if (bl.mode == 2) {
        int *state = bl.d_state ? bl.d_state : Workspace::get<int>(BALANCE_STATE_WORDS); // scratch: every frame on its own
        uint32_t *hist = Workspace::get<uint32_t>(BALANCE_HIST_WORDS);
        launch_balance_measure(state, hist, &in, nullptr, nullptr, H, W, elem_sz, bl.max_shift, balance_rate_q(bl.rate), bl.d_state == nullptr);
        st = state;
    }
    const u8 *lut = st ? nullptr : bl.lut;
    u8 *out = Workspace::get<u8>(2 * IMG);
    launch_balance_frame(out, &in, nullptr, H, W, elem_sz, lut, st);
    prev_out = nullptr;
    if (prev_frame) {
        PackInput prev = in;
        prev.frame = prev_frame;
        u8 *po = Workspace::get<u8>(2 * IMG);
        launch_balance_frame(po, &prev, nullptr, H, W, elem_sz, lut, st);
        prev_out = po;
    }
    return out;
}

// ---- the shot-change detector of a frame call's input (stm_set_cut), ahead of the alignment's measurement
// the thread's setting against a frame call's geometry; off: nothing to check, the call is as it was
bool frame_cut_ok(const char *fn, int num_rows, int num_cols) { return !cut().mode || cut_size_ok(fn, num_rows, num_cols); }
size_t cut_ws_bytes() { return CUT_SIG_WORDS * 4 + 512; }
// The prelude, inside the frame call's Workspace scope, first of all: the three launches on the screened full-resolution frame `in`.
// The reset pointers are the caller's states of depth mode 2 (where the call renders), alignment mode 2 and balance mode 2; a null
// one is scratch memory and has no history to lose.
void cut_frame_input(const Cut &ct, const PackInput &in, int H, int W, int elem_sz, bool renders, const Align &aln, const Balance &bal)
{
    const Depth dp = depth();
    uint32_t *sig = Workspace::get<uint32_t>(CUT_SIG_WORDS);
    launch_cut_detect(ct.d_state, sig, &in, nullptr, H, W, elem_sz, ct.thresh_permille, ct.min_gap,
                      renders && dp.mode == 2 ? (void *)dp.d_state : nullptr, aln.mode == 2 ? (void *)aln.d_state : nullptr,
                      bal.mode == 2 ? (void *)bal.d_state : nullptr);
}

// ---- the active picture area of a frame call's input (stm_set_active), after the cut detector and before the alignment
// the thread's setting against a frame call's geometry; off: nothing to check, the call is as it was
bool frame_active_ok(const char *fn, int num_rows, int num_cols)
{
    const Active ac = active();
    if (!ac.mode) return true;
    return ac.mode == 1 ? active_rect_ok(fn, ac.rect, num_rows, num_cols) : active_size_ok(fn, num_rows, num_cols);
}
// the counts, a scratch state and the rectangle's four words
size_t active_ws_bytes(int num_rows, int num_cols) { return ((size_t)num_rows + num_cols + ACTIVE_STATE_WORDS + 4) * 4 + 1024; }
// The prelude, inside the frame call's Workspace scope: mode 2 runs the three launches on the screened full-resolution frame `in`
// (the left eye is the reference of the alignment and the balance, so the result depends on neither) and the rectangle is the
// state's words 1 .. 4; mode 1 writes the given rectangle into four workspace words.  Either way the consumers read it on the device.
const int *active_frame_input(const Active &ac, const Cut &ct, const PackInput &in, int H, int W, int elem_sz)
{
    if (ac.mode == 1) {
        int *rect = Workspace::get<int>(4);
        launch_active_rect(rect, ac.rect);
        return rect;
    }
    int *state = ac.d_state ? ac.d_state : Workspace::get<int>(ACTIVE_STATE_WORDS); // scratch: every frame on its own
    uint32_t *counts = Workspace::get<uint32_t>((size_t)H + W);
    launch_active_detect(state, counts, &in, nullptr, H, W, elem_sz, ac.thresh_luma, ac.lit_permille, ac.max_bar_permille, ac.hold,
                         ac.d_state == nullptr, ct.mode ? ct.d_state : nullptr);
    return state + 1;
}
// with `fill` on, both maps a frame call hands back take fill_disp outside the rectangle: after the temporal step, before the tail
void frame_active_fill(const int *d_rect, float *d_disp_l, float *d_disp_r, int H, int W)
{
    const Active ac = active();
    if (!ac.mode || !ac.fill || !d_rect) return;
    float *m[2] = {d_disp_l, d_disp_r};
    launch_active_fill(2, m, H, W, d_rect, ac.fill_disp);
}

// ---- the input prelude of a frame call: the thread's shot-change detector, alignment and balance ahead of the front
// the three settings against a frame call's geometry, alignment first; nv: the call's NV12 input or null
bool frame_settings_ok(const char *fn, const FrameArgs &a, const Nv12Input *nv)
{
    const bool bgr_sbs = !nv && !packing().on(); // both eyes are gathered from a side-by-side BGR frame
    return frame_rectify_ok(fn, a.num_cols_sbs, a.num_cols, bgr_sbs) && frame_align_ok(fn, a.num_rows, a.num_cols_sbs, a.num_cols, bgr_sbs) &&
           frame_balance_ok(fn, a.num_rows, a.num_cols_sbs, a.num_cols, bgr_sbs) && frame_cut_ok(fn, a.num_rows, a.num_cols) &&
           frame_active_ok(fn, a.num_rows, a.num_cols);
}
// what the thread's settings add to a frame body's Workspace::begin; prev: a side-by-side history goes through the prelude too
size_t frame_settings_ws_bytes(const FrameArgs &a, bool prev)
{
    const size_t IMG = (size_t)a.num_rows * a.num_cols * a.elem_sz;
    return (output().format == 1 ? (size_t)a.num_rows_out * a.num_cols_out * a.elem_sz : 0) + // the un-fused NV12 frame's BGR quilt
           (antialias().mode == 1 ? 2 * IMG + 512 : 0) +                                       // the prefiltered pair
           (rectify().mode ? rectify_ws_bytes(IMG, prev) : 0) +                                // the rectified frame(s)
           (align().mode ? align_ws_bytes(a.num_rows, IMG, prev) : 0) +                        // the aligned frame(s)
           (balance().mode ? balance_ws_bytes(IMG, prev) : 0) +                                // the balanced frame(s)
           (cut().mode ? cut_ws_bytes() : 0) +                                                 // the detector's signature
           (active().mode ? active_ws_bytes(a.num_rows, a.num_cols) : 0) +                     // the active area's counts, state and rectangle
           (overlay().mode == 1 && overlay_auto().mode == 1 ? OVERLAY_FIT_WS_WORDS * 4 + 16 + 1024 : 0); // the overlay fit's bins, box and scratch state
}
// what the front and the temporal step of a frame body read, after the prelude
struct FrameInput {
    const u8 *d_img_sbs; // the side-by-side BGR frame (the caller's, or the aligned / balanced one in the workspace), null for NV12
    int num_cols_sbs;
    const Nv12Input *nv;    // the NV12 planes, null once a setting has converted them
    const u8 *prev_sbs;     // the history's side-by-side frame, through THIS frame's field and tables; null without one
    bool pack_on;           // the frame is still packed: the front unpacks it
    bool split_hist;        // an NV12 call: its history comes as split images, used as they are passed
    PackInput pin;          // the frame as the call was given it
    const int *rect;        // the active rectangle's four words in device memory (stm_set_active), null with the setting off
};
// The prelude, inside the frame call's Workspace scope and after the split images (and the reduced pair) have been carved: the
// rectification, then cut, active area, align and balance, each where its setting is on.  After a rectification every later step
// sees the plain BGR frame call on the rectified pair.  After an alignment or a balance the call is the plain BGR frame call on
// the prepared side-by-side frame, and a side-by-side history has gone through the same field and tables.
FrameInput frame_input(const FrameArgs &a, const u8 *d_img_sbs, const Nv12Input *nv, const TemporalHist *hist)
{
    const int H = a.num_rows, W = a.num_cols, elem_sz = a.elem_sz;
    const Packing pack = packing(); // a packed frame (stm_set_packing): the caller has screened its geometry, or refused it
    const Align aln = align();
    const Balance bal = balance();
    const Cut ct = cut();
    FrameInput in = {d_img_sbs, a.num_cols_sbs, nv, hist ? hist->sbs : nullptr, pack.on() && !aln.mode && !bal.mode, nv != nullptr,
                     {pack, nv != nullptr, d_img_sbs, a.num_cols_sbs, nv ? nv->y : nullptr, nv ? nv->uv : nullptr, nv ? nv->pitch_y : 0,
                      nv ? nv->pitch_uv : 0, nv ? nv->matrix : 0}, nullptr};
    const bool sbs_hist = hist && !in.split_hist;
    const Rectify rc = rectify();
    if (rc.mode) { // first of all: from here on the call is the plain BGR frame call on the rectified side-by-side frame
        const u8 *prev = nullptr;
        in.d_img_sbs = rectify_frame_input(rc, in.pin, sbs_hist ? in.prev_sbs : nullptr, H, W, elem_sz, prev);
        if (sbs_hist) in.prev_sbs = prev;
        in.pin = PackInput{Packing{0, 0, 0, 0}, false, in.d_img_sbs, 2 * W, nullptr, nullptr, 0, 0, 0};
        in.num_cols_sbs = 2 * W;
        in.nv = nullptr;
        in.pack_on = false;
    }
    if (ct.mode) cut_frame_input(ct, in.pin, H, W, elem_sz, (a.stages & 0xff) >= 3, aln, bal); // before any state's fit runs
    const Active ac = active();
    in.rect = ac.mode ? active_frame_input(ac, ct, in.pin, H, W, elem_sz) : nullptr; // after the cut flag, on the input as given
    if (aln.mode) { // from here on the call is the plain BGR frame call on the aligned side-by-side frame
        const u8 *prev = nullptr;
        in.d_img_sbs = align_frame_input(aln, in.pin, sbs_hist ? in.prev_sbs : nullptr, H, W, elem_sz, prev);
        if (sbs_hist) in.prev_sbs = prev;
    }
    if (bal.mode) { // after the alignment, on whatever the call now points at; then it is the plain BGR frame call on the balanced frame
        const PackInput plain = {Packing{0, 0, 0, 0}, false, in.d_img_sbs, 2 * W, nullptr, nullptr, 0, 0, 0};
        const u8 *prev = nullptr;
        in.d_img_sbs = balance_frame_input(bal, aln.mode ? plain : in.pin, sbs_hist ? in.prev_sbs : nullptr, H, W, elem_sz, prev);
        if (sbs_hist) in.prev_sbs = prev;
    }
    if (aln.mode || bal.mode) {
        in.num_cols_sbs = 2 * W;
        in.nv = nullptr;
    }
    return in;
}

// temporal stabilisation (0x2000): the final maps pulled towards the previous frame's where neither colour nor disparity moved, each
// view on its own half of the two side-by-side buffers (read in place: the history was never split) -- or, for an NV12 or a packed
// frame, on the two frames' split images
void frame_temporal(const FrameArgs &a, const FrameInput &in, const TemporalHist &hist, const u8 *img_l, const u8 *img_r, float *d_disp_l,
                    float *d_disp_r)
{
    const int H = a.num_rows, W = a.num_cols, elem_sz = a.elem_sz;
    float *c[2] = {d_disp_l, d_disp_r};
    const float *q[2] = {hist.disp_l, hist.disp_r};
    const bool split = in.split_hist || in.pack_on; // the views as split images; otherwise in place in the two side-by-side frames
    const u8 *prev_l = hist.img_l, *prev_r = hist.img_r;
    if (in.pack_on && !in.nv) { // the previous PACKED frame: its images are its unpacking (one more launch in this combination only)
        const size_t IMG = (size_t)H * W * elem_sz;
        u8 *ul = Workspace::get<u8>(IMG), *ur = Workspace::get<u8>(IMG);
        PackInput prev = in.pin;
        prev.frame = in.prev_sbs;
        launch_demux_packed(ul, ur, prev, H, W, elem_sz);
        prev_l = ul;
        prev_r = ur;
    }
    const u8 *im[2] = {split ? img_l : in.d_img_sbs, split ? img_r : in.d_img_sbs}, *ip[2] = {split ? prev_l : in.prev_sbs, split ? prev_r : in.prev_sbs};
    const size_t off[2] = {0, split ? 0 : (size_t)W * elem_sz};
    launch_disp_temporal(2, c, q, im, ip, off, H, W, split ? W : in.num_cols_sbs, elem_sz, hist.alpha, hist.thresh_color, hist.thresh_disp);
}

// the tail of a rendering frame call: the renderer, then the thread's overlay (stm_set_overlay) composited on the finished frame --
// the call's last launch.  With stm_set_overlay_auto on, the overlay's disparity is first fitted to the maps the renderer read, under
// the depth budget it rendered with and the thread's cut state, and the compositor reads it from the state on the device
// d_rect: the active rectangle the two fits read on the device (stm_set_active), or null
void frame_tail(const FrameArgs &a, u8 *img_l, u8 *img_r, float *d_disp_l, float *d_disp_r, u8 *d_interlaced, const int *d_rect)
{
    float *depth_state = nullptr;
    frame_render(img_l, img_r, d_disp_l, d_disp_r, d_interlaced, a, &depth_state, d_rect);
    if (overlay().mode != 1) return;
    const OverlayAuto oa = overlay_auto();
    if (oa.mode != 1) {
        frame_overlay(d_interlaced, overlay(), lens(), layout(), a.num_views, a.angle, a.num_rows_out, a.num_cols_out, a.elem_sz);
        return;
    }
    uint32_t *ws = Workspace::get<uint32_t>(OVERLAY_FIT_WS_WORDS);
    float *state = oa.d_state ? oa.d_state : Workspace::get<float>(4); // scratch: zeroed, every frame on its own
    const Cut ct = cut();
    frame_overlay_auto(d_interlaced, overlay(), oa, state, ws, oa.d_state == nullptr, oa.d_state == nullptr, d_disp_l, d_disp_r, a.num_rows,
                       a.num_cols, depth(), depth_state, ct.mode ? ct.d_state : nullptr, lens(), layout(), a.num_views, a.angle, a.num_rows_out,
                       a.num_cols_out, a.elem_sz, d_rect);
}

// the body of stm_d_adcensus_stm, stm_d_adcensus_stm_t and stm_d_adcensus_stm_nv12; hist != nullptr: the temporal step between
// the bilateral filter and the renderer; nv != nullptr: the frame comes as NV12 planes (d_img_sbs is null, num_cols_sbs >= 2 W).
// Every argument has been screened by the caller except the `stages` rules the calls share.
void frame_device(const char *fn, const FrameArgs &a, const u8 *d_img_sbs, float *d_disp_l, float *d_disp_r, u8 *d_interlaced,
                  const TemporalHist *hist, const Nv12Input *nv = nullptr)
{
    const int stages = a.stages;
    if ((stages & 0x300) == 0x300) // sub-pixel enhancement reads the last horizontal pass's input, which HSLO does not keep
        return (void)STM_REJECT("stages", "%s: stages 0x200 (sub-pixel) together with 0x100 (HSLO) is not supported", fn);
    if ((stages & 0x400) && (stages & 0xff) < 2) // interpolation fills what the L/R check marked: stage 1 has no outlier maps
        return (void)STM_REJECT("stages", "%s: stages 0x400 (outlier interpolation) needs the refinement stages (2 or 3)", fn);
    if ((stages & 0x800) && (stages & 0xff) < 3) // linear sampling changes the renderer only: stages 1 and 2 render nothing
        return (void)STM_REJECT("stages", "%s: stages 0x800 (linear sampling of the warps) needs the rendering stage (3)", fn);
    if (stages & 0x1000) // guided up-sampling belongs to the reduced-resolution frame: here nothing is up-scaled
        return (void)STM_REJECT("stages", "%s: stages 0x1000 (guided disparity up-sampling) needs the reduced-resolution frame (d_adcensus_stm_2s)", fn);
    if (!frame_layout_ok(fn, a) || !frame_settings_ok(fn, a, nv)) return;
    const int H = a.num_rows, W = a.num_cols, N = a.num_views, elem_sz = a.elem_sz;
    const size_t HW = (size_t)H * W, IMG = HW * elem_sz;
    const size_t V = pq_volume_floats(a.num_disp, H, W); // >= the quad-interleaved volume of the HSLO / legacy paths
    const bool unpacked_hist = packing().on() && hist && !nv; // the previous packed frame's two images (frame_temporal)
    Workspace::begin(((stages & 0x100) ? 13 : 4) * V * 4 + (size_t)(N + 2 + (unpacked_hist ? 2 : 0)) * IMG + 168 * HW + (1u << 20) +
                     frame_settings_ws_bytes(a, hist && !nv));
    const bool own_img = nv && nv->img_l; // the caller keeps the split images (the next frame's history)
    u8 *img_l = own_img ? nv->img_l : Workspace::get<u8>(IMG), *img_r = own_img ? nv->img_r : Workspace::get<u8>(IMG);
    uint32_t *pre[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const FrameInput in = frame_input(a, d_img_sbs, nv, hist);
    nv = in.nv;
    bool fused_split = in.num_cols_sbs >= 2 * W; // both halves complete: emit the derived pixel formats in the same pass
    if (in.pack_on && (agg_variant() / 100) % 10 != 6) { // the gather, the filter and the conversion in stm_k_front's pass
        for (int i = 0; i < 6; ++i) pre[i] = Workspace::get<uint32_t>(HW);
        launch_front_pack(img_l, img_r, pre[0], pre[1], pre[2], pre[3], pre[4], pre[5], in.pin, H, W, elem_sz);
        fused_split = true;
    } else if (in.pack_on) { // 600: the plain unpacking, then the pixel formats and the census as kernels of their own
        launch_demux_packed(img_l, img_r, in.pin, H, W, elem_sz);
        fused_split = false;
    } else if (nv && (agg_variant() / 100) % 10 != 6) { // the conversion in stm_k_front's pass
        for (int i = 0; i < 6; ++i) pre[i] = Workspace::get<uint32_t>(HW);
        launch_front_nv12(img_l, img_r, pre[0], pre[1], pre[2], pre[3], pre[4], pre[5], nv->y, nv->pitch_y, nv->uv, nv->pitch_uv, H, W,
                          elem_sz, nv->matrix);
    } else if (nv) { // 600: the plain converter, then the pixel formats and the census as kernels of their own
        launch_demux_nv12(img_l, img_r, nv->y, nv->pitch_y, nv->uv, nv->pitch_uv, H, W, elem_sz, nv->matrix);
        fused_split = false;
    } else if (fused_split && (agg_variant() / 100) % 10 != 6) { // ... and the census words; 600: the split and the census as two kernels
        for (int i = 0; i < 6; ++i) pre[i] = Workspace::get<uint32_t>(HW);
        launch_front(img_l, img_r, pre[0], pre[1], pre[2], pre[3], pre[4], pre[5], in.d_img_sbs, H, in.num_cols_sbs, W, elem_sz);
    } else if (fused_split) {
        for (int i = 0; i < 4; ++i) pre[i] = Workspace::get<uint32_t>(HW);
        launch_demux_sbs_packed(img_l, img_r, pre[0], pre[1], pre[2], pre[3], in.d_img_sbs, H, in.num_cols_sbs, W, elem_sz);
    } else {
        launch_demux_sbs(img_l, img_r, in.d_img_sbs, H, in.num_cols_sbs, W, elem_sz);
    }
    frame_disparity(img_l, img_r, d_disp_l, d_disp_r, H, W, a, (stages & 0xff) >= 2, fused_split ? pre : nullptr);
    if (hist) frame_temporal(a, in, *hist, img_l, img_r, d_disp_l, d_disp_r);
    frame_active_fill(in.rect, d_disp_l, d_disp_r, H, W);
    if ((stages & 0xff) >= 3) frame_tail(a, img_l, img_r, d_disp_l, d_disp_r, d_interlaced, in.rect);
}

// ---- the screens of the frame entries
bool frame_dims_ok(const char *fn, const FrameArgs &a)
{
    return args_ok(fn, {{"num_rows", a.num_rows, 1}, {"num_cols_sbs", a.num_cols_sbs, 1}, {"num_cols", a.num_cols, 1},
                        {"num_rows_out", a.num_rows_out, 1}, {"num_cols_out", a.num_cols_out, 1}, {"elem_sz", a.elem_sz, 3},
                        {"num_views", a.num_views, 2}, {"num_disp", a.num_disp, 1}});
}

// the thread's packing (stm_set_packing) against a BGR frame call's geometry; packing off: nothing to check, the call is as it was
bool frame_packing_ok(const char *fn, const FrameArgs &a)
{
    const Packing pk = packing();
    return !pk.on() || packing_args_ok(fn, pk, a.num_rows, a.num_cols_sbs, a.num_cols, "num_cols", false, 0, 0, 0);
}
// the calls that take the reference's layout only
bool packing_unsupported(const char *fn)
{
    if (!packing().on()) return false;
    return !STM_REJECT("packing", "%s: a packing is set on this thread (stm_set_packing), which this call does not support: use d_adcensus_stm, "
                       "d_adcensus_stm_t or d_adcensus_stm_nv12", fn);
}

// the two output images of an NV12 call come together or not at all
bool nv12_images_ok(const char *fn, const Nv12Input &nv)
{
    if ((nv.img_l != nullptr) == (nv.img_r != nullptr)) return true;
    return STM_REJECT("d_img_l, d_img_r", "%s: d_img_l and d_img_r must be both null (the split images stay in the workspace) or both set", fn);
}

// `stages` bit 0x2000 of the four entries that take a history: the three parameters, then the pointers.  nv == nullptr: the
// side-by-side form (the previous frame and its two maps), else the split form of the NV12 entries (the previous split images and
// maps, and this frame's images kept by the caller).  *run: all history pointers are set, so the step runs (all null: the first
// frame of a sequence).  The rule for stages below 2 can fire for the full-resolution entries only: the reduced ones always render.
bool frame_history_ok(const char *fn, const FrameArgs &a, const TemporalHist &h, const float *d_disp_l, const float *d_disp_r,
                      const Nv12Input *nv, bool *run)
{
    *run = false;
    if (!(a.stages & 0x2000)) return true;
    if (!temporal_params_ok(fn, h.alpha, h.thresh_color, h.thresh_disp)) return false;
    const bool split = nv != nullptr;
    const size_t HW = (size_t)a.num_rows * a.num_cols, IMG = HW * a.elem_sz;
    // the history is read while the outputs are written: images first, then maps
    const void *hp[4] = {h.img_l, h.img_r, h.disp_l, h.disp_r}, *out[4] = {split ? nv->img_l : nullptr, split ? nv->img_r : nullptr, d_disp_l, d_disp_r};
    const size_t sz[4] = {IMG, IMG, HW * 4, HW * 4};
    const int first = split ? 0 : 2, all = split ? 4 : 3;
    const int nset = (split ? (h.img_l != nullptr) + (h.img_r != nullptr) : (h.sbs != nullptr)) + (h.disp_l != nullptr) + (h.disp_r != nullptr);
    bool alias = false;
    for (int i = first; i < 4 && nset == all; ++i)
        for (int j = first; j < 4; ++j) alias = alias || bytes_overlap(hp[i], sz[i], out[j], sz[j]);
    if ((a.stages & 0xff) < 2) // the step filters the refined maps: stage 1 has none
        return STM_REJECT("stages", "%s: stages 0x2000 (temporal stabilisation) needs the refinement stages (2 or 3)", fn);
    if (split && !nv->img_l) // this frame's converted images are the next frame's history: the caller must keep them
        return STM_REJECT("d_img_l, d_img_r", "%s: stages 0x2000 (temporal stabilisation) needs the output images d_img_l and d_img_r", fn);
    if (nset != 0 && nset != all)
        return STM_REJECT(split ? "d_prev_img_l, d_prev_img_r, d_prev_disp_l, d_prev_disp_r" : "d_prev_img_sbs, d_prev_disp_l, d_prev_disp_r",
                          "%s: the %s history pointers must be all null (first frame) or all set", fn, split ? "four" : "three");
    if (nset == all && !split && !packing().on() && a.num_cols_sbs < 2 * a.num_cols) // the views are read from the two halves in place
        return STM_REJECT("num_cols_sbs", "%s: stages 0x2000 (temporal stabilisation) needs num_cols_sbs >= 2 * num_cols", fn);
    if (alias && split)
        return STM_REJECT("d_prev_img_l, d_prev_img_r, d_prev_disp_l, d_prev_disp_r",
                          "%s: a history buffer must not alias an output (d_img_l, d_img_r, d_disp_l, d_disp_r)", fn);
    if (alias) return STM_REJECT("d_prev_disp_l, d_prev_disp_r", "%s: a history map must not alias d_disp_l or d_disp_r", fn);
    *run = nset == all;
    return true;
}

// adcensus_stm_2, d_io.cu:240-508: the disparity is computed on a bilinearly reduced pair
// (num_rows_disp x num_cols_disp, tx_scale_bilinear_kernel :302-304), scaled back up with
// tx_disp_scale_kernel(1/disp_scale) (:415-417), then the views are rendered at full resolution.
// The two _2s calls add the `stages` word (stm_hip.h); the two reference calls are the same bodies with stages = 3.

// the screen of every reduced-resolution entry, once per call; temporal_ok: the call has the history arguments of stages bit
// 0x2000 (d_adcensus_stm_2t, d_adcensus_stm_2nv12)
bool reduced_args_ok(const char *fn, const FrameArgs &a, bool temporal_ok = false)
{
    if (!args_ok(fn, {{"num_rows", a.num_rows, 1}, {"num_cols_sbs", a.num_cols_sbs, 1}, {"num_cols", a.num_cols, 1},
                      {"num_rows_out", a.num_rows_out, 1}, {"num_cols_out", a.num_cols_out, 1}, {"num_rows_disp", a.num_rows_disp, 1},
                      {"num_cols_disp", a.num_cols_disp, 1}, {"elem_sz", a.elem_sz, 3}, {"num_views", a.num_views, 2},
                      {"num_disp", a.num_disp, 1}}))
        return false;
    if (packing_unsupported(fn)) return false;
    const int stages = a.stages;
    if ((stages & 0xff) != 3 || (stages & ~(temporal_ok ? 0x3fff : 0x1fff))) // this path always renders
        return STM_REJECT("stages", "%s: stages = 0x%x, must be 3, optionally OR-ed with 0x100, 0x200, 0x400, 0x800%s 0x1000%s", fn, stages,
                          temporal_ok ? "," : " and", temporal_ok ? " and 0x2000" : "");
    if ((stages & 0x300) == 0x300) // as d_adcensus_stm
        return STM_REJECT("stages", "%s: stages 0x200 (sub-pixel) together with 0x100 (HSLO) is not supported", fn);
    return true;
}

// the reduced pair's front as the parent of stm_k_front_low ran it and as narrow frames and stm_set_agg_variant(600) still do: the
// split (NV12: the plain converter) and one reduction per view; the pixel formats and the census follow in frame_disparity
void reduced_front_chain(u8 *img_l, u8 *img_r, u8 *low_l, u8 *low_r, const u8 *d_img_sbs, int num_cols_sbs, const Nv12Input *nv, int H, int W,
                         int h, int w, int elem_sz)
{
    if (nv) launch_demux_nv12(img_l, img_r, nv->y, nv->pitch_y, nv->uv, nv->pitch_uv, H, W, elem_sz, nv->matrix);
    else launch_demux_sbs(img_l, img_r, d_img_sbs, H, num_cols_sbs, W, elem_sz);
    launch_scale_bilinear(img_l, low_l, H, W, h, w, elem_sz);
    launch_scale_bilinear(img_r, low_r, H, W, h, w, elem_sz);
}
bool reduced_front_fused(int num_cols_sbs, int W) { return num_cols_sbs >= 2 * W && (agg_variant() / 100) % 10 != 6; }

// the body of the reduced-resolution frame calls, screened by the caller (reduced_args_ok); hist != nullptr: the temporal step on
// the up-scaled full-size maps, between the up-scale and the renderer (the placement rule of frame_device: on the final maps);
// nv != nullptr: the frame comes as NV12 planes (d_img_sbs is null, num_cols_sbs >= 2 W)
void reduced_frame_device(const char *fn, const FrameArgs &a, const u8 *d_img_sbs, float *d_disp_l, float *d_disp_r, u8 *d_interlaced,
                          const TemporalHist *hist, const Nv12Input *nv = nullptr)
{
    if (!frame_layout_ok(fn, a) || !frame_settings_ok(fn, a, nv)) return;
    const int H = a.num_rows, W = a.num_cols, h = a.num_rows_disp, w = a.num_cols_disp, N = a.num_views, elem_sz = a.elem_sz;
    const size_t HW = (size_t)H * W, IMG = HW * elem_sz, hw = (size_t)h * w;
    const size_t V = pq_volume_floats(a.num_disp, h, w);
    Workspace::begin((stages_hslo(a.stages) ? 13 : 4) * V * 4 + (size_t)(N + 4) * IMG + 136 * HW + 32 * hw + (1u << 20) + // HSLO: as d_adcensus_stm
                     frame_settings_ws_bytes(a, hist && !nv));
    const bool own_img = nv && nv->img_l; // the caller keeps the split images (the next frame's history)
    u8 *img_l = own_img ? nv->img_l : Workspace::get<u8>(IMG), *img_r = own_img ? nv->img_r : Workspace::get<u8>(IMG);
    u8 *low_l = Workspace::get<u8>(hw * elem_sz), *low_r = Workspace::get<u8>(hw * elem_sz);
    const FrameInput in = frame_input(a, d_img_sbs, nv, hist); // on the full-resolution input
    nv = in.nv;
    uint32_t *pre[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const bool fused = reduced_front_fused(in.num_cols_sbs, W); // both halves complete; 600: the chain of kernels
    {
        ProfScope p("reduced_front");
        if (fused) { // the split, both reductions, the reduced pair's pixel formats and census words in one launch
            for (int i = 0; i < 6; ++i) pre[i] = Workspace::get<uint32_t>(hw);
            launch_front_low(img_l, img_r, low_l, low_r, pre[0], pre[1], pre[2], pre[3], pre[4], pre[5], nv ? nullptr : in.d_img_sbs,
                             in.num_cols_sbs, nv ? nv->y : nullptr, nv ? nv->pitch_y : 0, nv ? nv->uv : nullptr, nv ? nv->pitch_uv : 0,
                             nv ? nv->matrix : 0, H, W, h, w, elem_sz);
        } else {
            reduced_front_chain(img_l, img_r, low_l, low_r, in.d_img_sbs, in.num_cols_sbs, nv, H, W, h, w, elem_sz);
        }
    }
    float *low_dl = Workspace::get<float>(hw), *low_dr = Workspace::get<float>(hw);
    frame_disparity(low_l, low_r, low_dl, low_dr, h, w, a, true, fused ? pre : nullptr); // HSLO, sub-pixel, interpolation: on the reduced pair
    const float up = 1.0f / a.disp_scale; // :415
    if (a.stages & 0x1000) { // guided: each map by its own view, the full-size image the views are rendered from against the image the match ran on
        float *o[2] = {d_disp_l, d_disp_r};
        const float *dl[2] = {low_dl, low_dr};
        const u8 *il[2] = {low_l, low_r}, *im[2] = {img_l, img_r};
        launch_disp_upsample(2, o, dl, il, im, upsample_table(15.0f), H, W, h, w, elem_sz, up);
    } else {
        launch_disp_scale(d_disp_l, low_dl, H, W, h, w, up);
        launch_disp_scale(d_disp_r, low_dr, H, W, h, w, up);
    }
    if (hist) frame_temporal(a, in, *hist, img_l, img_r, d_disp_l, d_disp_r);
    frame_active_fill(in.rect, d_disp_l, d_disp_r, H, W);
    frame_tail(a, img_l, img_r, d_disp_l, d_disp_r, d_interlaced, in.rect);
}

// the host flavour of the reference's three frame calls: the screens, before the caller's arrays are written; the arrays staged in
// the thread's cached buffers (outside the workspace: the body re-carves it); the device body; the three arrays copied back
void frame_host(const char *fn, const FrameArgs &a, bool reduced, const u8 *img_sbs, float *disp_l, float *disp_r, u8 *interlaced)
{
    if (reduced ? !reduced_args_ok(fn, a) : !frame_dims_ok(fn, a) || packing_unsupported(fn)) return;
    if (!frame_layout_ok(fn, a) || !frame_settings_ok(fn, a, nullptr)) return;
    const size_t HW = (size_t)a.num_rows * a.num_cols, sbs_sz = (size_t)a.num_rows * a.num_cols_sbs * a.elem_sz;
    const size_t out_sz = frame_out_bytes(a.num_rows_out, a.num_cols_out, a.elem_sz); // stm_set_output: the NV12 surface
    const size_t need[4] = {sbs_sz, out_sz, HW * 4, HW * 4};
    void *buf[4];
    if (!host_frame_bufs(need, buf)) return;
    u8 *d_sbs = (u8 *)buf[0], *d_out = (u8 *)buf[1];
    float *d_dl = (float *)buf[2], *d_dr = (float *)buf[3];
    STM_CHECK(hipMemcpyAsync(d_sbs, img_sbs, sbs_sz, hipMemcpyHostToDevice, stream()));
    STM_CHECK(hipMemsetAsync(d_out, 0, out_sz, stream()));
    ApiNest nest; // the device body must not forget a failed upload
    (reduced ? reduced_frame_device : frame_device)(fn, a, d_sbs, d_dl, d_dr, d_out, nullptr, nullptr);
    down(disp_l, d_dl, HW); down(disp_r, d_dr, HW); down(interlaced, d_out, out_sz);
    sync();
}

// the reference's frame parameters under the names every extern "C" frame entry gives them, in FrameArgs' order: the one place
// where that order is written out
#define STM_FRAME_PARAMS                                                                                                                  \
    num_rows, num_cols_sbs, num_cols, num_rows_out, num_cols_out, elem_sz, num_views, angle, num_disp, zero_disp, ad_coeff, census_coeff, \
        ucd, lcd, usd, lsd, thresh_s, thresh_h

} // namespace

// The body of a frame stream's image-plus-depth frame (stm_stream_input_depth, step F of its definition): frame_device without the
// front and the matcher.  The cut and the active-area detector run on the given image as the left eye, ahead of the kernel, as
// frame_input runs them; stm_k_eye decodes the plane into d_disp_l and synthesises the right image and d_disp_r; then the active fill
// and frame_tail exactly as the stereo body calls them.  The stream has screened the plane's arguments and keeps the settings that
// condition a stereo pair (packing, alignment, balance, NV12 input, a match size) off.  Not an extern "C" entry: see stm_common.h
void stm::depth_frame_device(const u8 *d_img, const void *d_plane, const DepthInput &di, float *d_disp_l, float *d_disp_r, u8 *d_interlaced,
                             int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out, int elem_sz, int num_views,
                             float angle, int stages)
{
    const char *fn = "stream_input_depth";
    const FrameArgs a = {num_rows, num_cols_sbs, num_cols, num_rows_out, num_cols_out, elem_sz, num_views, angle, 1, 0, 0.0f, 0.0f, 0.0f, 0.0f,
                         0, 0, 0, 0.0f, stages};
    if (!frame_dims_ok(fn, a)) return;
    if ((stages & ~0x800) != 3) return (void)STM_REJECT("stages", "%s: stages = 0x%x, must be 3 or 3 | 0x800 (nothing is matched)", fn, stages);
    if (num_cols > 8192) return (void)STM_REJECT("num_cols", "%s: num_cols = %d, must be <= 8192 (a row's keys live in LDS)", fn, num_cols);
    if (num_cols_sbs < num_cols) return (void)STM_REJECT("num_cols_sbs", "%s: num_cols_sbs = %d, must be >= num_cols = %d", fn, num_cols_sbs, num_cols);
    if (!frame_layout_ok(fn, a) || !frame_cut_ok(fn, num_rows, num_cols) || !frame_active_ok(fn, num_rows, num_cols)) return;
    const int H = num_rows, W = num_cols;
    const size_t HW = (size_t)H * W, IMG = HW * elem_sz;
    // the two images, the tail's masks, views and tables; no volumes
    Workspace::begin((size_t)(num_views + 2) * IMG + 40 * HW + (1u << 20) + frame_settings_ws_bytes(a, false));
    u8 *img_r = Workspace::get<u8>(IMG), *img_l = num_cols_sbs > W ? Workspace::get<u8>(IMG) : nullptr;
    const PackInput pin = {Packing{0, 0, 0, 0}, false, d_img, num_cols_sbs, nullptr, nullptr, 0, 0, 0};
    const Cut ct = cut();
    if (ct.mode) cut_frame_input(ct, pin, H, W, elem_sz, true, align(), balance()); // before any state's fit runs
    const Active ac = active();
    const int *rect = ac.mode ? active_frame_input(ac, ct, pin, H, W, elem_sz) : nullptr;
    launch_depth_eye(d_img, num_cols_sbs, d_plane, di.format, di.lo, di.hi, di.fill, di.gate, img_l, img_r, d_disp_l, d_disp_r, H, W, elem_sz);
    frame_active_fill(rect, d_disp_l, d_disp_r, H, W);
    frame_tail(a, img_l ? img_l : const_cast<u8 *>(d_img), img_r, d_disp_l, d_disp_r, d_interlaced, rect);
}

// The body of a frame stream's packed 2D-plus-depth video frame (stm_stream_input_packed_depth, include/stm_depth_video.h):
// depth_frame_device with one packed BGR or NV12 frame in place of the image and the plane.  The cut and the active-area detector
// read the image half as the left eye through the PackInput they take from any packed stereo frame (eye 0 under dv.pk), so the depth
// half never reaches them; stm_k_eye_video unpacks and converts the image into the tight img_l, decodes the depth picture into
// d_disp_l and synthesises img_r and d_disp_r; then the active fill and frame_tail as above.  The stream has screened dv and the
// geometry (stm_stream_set_packing's rules) and keeps every setting that conditions a stereo pair off.  Not an extern "C" entry
void stm::depth_video_frame_device(const u8 *d_frame, const DepthVideo &dv, float *d_disp_l, float *d_disp_r, u8 *d_interlaced, int num_rows,
                                   int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out, int elem_sz, int num_views,
                                   float angle, int stages)
{
    const char *fn = "stream_input_packed_depth";
    const FrameArgs a = {num_rows, num_cols_sbs, num_cols, num_rows_out, num_cols_out, elem_sz, num_views, angle, 1, 0, 0.0f, 0.0f, 0.0f, 0.0f,
                         0, 0, 0, 0.0f, stages};
    if (!frame_dims_ok(fn, a)) return;
    if ((stages & ~0x800) != 3) return (void)STM_REJECT("stages", "%s: stages = 0x%x, must be 3 or 3 | 0x800 (nothing is matched)", fn, stages);
    if (num_cols > 8192) return (void)STM_REJECT("num_cols", "%s: num_cols = %d, must be <= 8192 (a row's keys live in LDS)", fn, num_cols);
    const bool nv12 = dv.format == 1;
    if (!packing_args_ok(fn, dv.pk, num_rows, num_cols_sbs, num_cols, "num_cols", nv12, num_cols_sbs, num_cols_sbs, dv.matrix)) return;
    if (!frame_layout_ok(fn, a) || !frame_cut_ok(fn, num_rows, num_cols) || !frame_active_ok(fn, num_rows, num_cols)) return;
    const int H = num_rows, W = num_cols;
    const size_t HW = (size_t)H * W, IMG = HW * elem_sz;
    Workspace::begin((size_t)(num_views + 2) * IMG + 40 * HW + (1u << 20) + frame_settings_ws_bytes(a, false));
    u8 *img_r = Workspace::get<u8>(IMG), *img_l = Workspace::get<u8>(IMG);
    const u8 *uv = d_frame + (size_t)dv.pk.rows_f(H) * num_cols_sbs;
    const PackInput pin = {dv.pk, nv12, nv12 ? nullptr : d_frame, num_cols_sbs, nv12 ? d_frame : nullptr, nv12 ? uv : nullptr,
                           nv12 ? num_cols_sbs : 0, nv12 ? num_cols_sbs : 0, nv12 ? dv.matrix : 0};
    const Cut ct = cut();
    if (ct.mode) cut_frame_input(ct, pin, H, W, elem_sz, true, align(), balance()); // before any state's fit runs
    const Active ac = active();
    const int *rect = ac.mode ? active_frame_input(ac, ct, pin, H, W, elem_sz) : nullptr;
    launch_depth_eye_video(pin, dv, img_l, img_r, d_disp_l, d_disp_r, H, W, elem_sz);
    frame_active_fill(rect, d_disp_l, d_disp_r, H, W);
    frame_tail(a, img_l, img_r, d_disp_l, d_disp_r, d_interlaced, rect);
}

extern "C" {

// which aggregation kernels a frame call with these arguments runs (stm_hip.h); no launch, no device
int stm_agg_path(int num_disp, int zero_disp, int num_rows, int num_cols, int usd, int stages)
{
    return frame_agg_path(num_disp, zero_disp, num_rows, num_cols, usd, stages);
}
// whether stm_k_pq_hc2 runs the first horizontal pass of such a call, as its parts per image row (stm_hip.h); no launch, no device
int stm_first_pass_path(int num_disp, int zero_disp, int num_rows, int num_cols, int usd, int stages)
{
    return frame_first_pass_path(num_disp, zero_disp, num_rows, num_cols, usd, stages);
}
// the order of the hypotheses inside a pixel's record of such a call's PX volumes, or -1 off PX (stm_hip.h); no launch, no device
int stm_px_order(int num_disp, int zero_disp, int num_rows, int num_cols, int usd, int stages)
{
    return frame_px_order(num_disp, zero_disp, num_rows, num_cols, usd, stages);
}

void stm_d_adcensus_stm(unsigned char *d_img_sbs, float *d_disp_l, float *d_disp_r, unsigned char *d_interlaced,
                        int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out, int elem_sz,
                        int num_views, float angle, int num_disp, int zero_disp, float ad_coeff, float census_coeff,
                        float ucd, float lcd, int usd, int lsd, int thresh_s, float thresh_h, int stages)
{
    const char *fn = "d_adcensus_stm";
    const FrameArgs a = {STM_FRAME_PARAMS, stages};
    if (!frame_dims_ok(fn, a) || !frame_packing_ok(fn, a)) return;
    if (stages & 0x2000) // temporal stabilisation needs the previous frame: this call has no arguments for it
        return (void)STM_REJECT("stages", "d_adcensus_stm: stages 0x2000 (temporal stabilisation) needs the history arguments of d_adcensus_stm_t");
    frame_device(fn, a, d_img_sbs, d_disp_l, d_disp_r, d_interlaced, nullptr);
}

// stm_d_adcensus_stm with the history of the temporal stabilisation (stm_hip.h)
void stm_d_adcensus_stm_t(unsigned char *d_img_sbs, float *d_disp_l, float *d_disp_r, unsigned char *d_interlaced,
                          int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out, int elem_sz,
                          int num_views, float angle, int num_disp, int zero_disp, float ad_coeff, float census_coeff,
                          float ucd, float lcd, int usd, int lsd, int thresh_s, float thresh_h, int stages,
                          unsigned char *d_prev_img_sbs, float *d_prev_disp_l, float *d_prev_disp_r, float alpha, int thresh_color,
                          float thresh_disp)
{
    const char *fn = "d_adcensus_stm_t";
    const FrameArgs a = {STM_FRAME_PARAMS, stages};
    if (!frame_dims_ok(fn, a) || !frame_packing_ok(fn, a)) return;
    const TemporalHist hist = {d_prev_img_sbs, d_prev_disp_l, d_prev_disp_r, alpha, thresh_color, thresh_disp};
    bool run = false;
    if (!frame_history_ok(fn, a, hist, d_disp_l, d_disp_r, nullptr, &run)) return;
    frame_device(fn, a, d_img_sbs, d_disp_l, d_disp_r, d_interlaced, run ? &hist : nullptr);
}

// stm_d_adcensus_stm_t on an NV12 frame (stm_hip.h): the same body, the conversion fused into its first kernel
void stm_d_adcensus_stm_nv12(unsigned char *d_y, int pitch_y, unsigned char *d_uv, int pitch_uv, int matrix, float *d_disp_l, float *d_disp_r,
                             unsigned char *d_interlaced, int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out,
                             int elem_sz, int num_views, float angle, int num_disp, int zero_disp, float ad_coeff, float census_coeff,
                             float ucd, float lcd, int usd, int lsd, int thresh_s, float thresh_h, int stages,
                             unsigned char *d_prev_img_l, unsigned char *d_prev_img_r, float *d_prev_disp_l, float *d_prev_disp_r, float alpha,
                             int thresh_color, float thresh_disp, unsigned char *d_img_l, unsigned char *d_img_r)
{
    const char *fn = "d_adcensus_stm_nv12";
    const FrameArgs a = {STM_FRAME_PARAMS, stages};
    if (!frame_dims_ok(fn, a)) return;
    if (packing().on()) { // a packed NV12 frame: the packing's own geometry rules in place of the side-by-side ones
        if (!packing_args_ok(fn, packing(), num_rows, num_cols_sbs, num_cols, "num_cols", true, pitch_y, pitch_uv, matrix)) return;
    } else if (!nv12_args_ok(fn, num_rows, num_cols_sbs, num_cols, "num_cols", pitch_y, pitch_uv, matrix)) return;
    const Nv12Input nv = {d_y, d_uv, pitch_y, pitch_uv, matrix, d_img_l, d_img_r};
    const TemporalHist hist = {nullptr, d_prev_disp_l, d_prev_disp_r, alpha, thresh_color, thresh_disp, d_prev_img_l, d_prev_img_r};
    bool run = false;
    if (!nv12_images_ok(fn, nv) || !frame_history_ok(fn, a, hist, d_disp_l, d_disp_r, &nv, &run)) return;
    frame_device(fn, a, nullptr, d_disp_l, d_disp_r, d_interlaced, run ? &hist : nullptr, &nv);
}

void stm_d_adcensus_stm_2(unsigned char *d_img_sbs, float *d_disp_l, float *d_disp_r, unsigned char *d_interlaced,
                          int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out,
                          int num_rows_disp, int num_cols_disp, int elem_sz, float disp_scale, int num_views, float angle,
                          int num_disp, int zero_disp, float ad_coeff, float census_coeff, float ucd, float lcd, int usd,
                          int lsd, int thresh_s, float thresh_h)
{
    const FrameArgs a = {STM_FRAME_PARAMS, 3, num_rows_disp, num_cols_disp, disp_scale};
    if (reduced_args_ok("d_adcensus_stm_2", a)) reduced_frame_device("d_adcensus_stm_2", a, d_img_sbs, d_disp_l, d_disp_r, d_interlaced, nullptr);
}
void stm_d_adcensus_stm_2s(unsigned char *d_img_sbs, float *d_disp_l, float *d_disp_r, unsigned char *d_interlaced,
                           int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out,
                           int num_rows_disp, int num_cols_disp, int elem_sz, float disp_scale, int num_views, float angle,
                           int num_disp, int zero_disp, float ad_coeff, float census_coeff, float ucd, float lcd, int usd,
                           int lsd, int thresh_s, float thresh_h, int stages)
{
    const FrameArgs a = {STM_FRAME_PARAMS, stages, num_rows_disp, num_cols_disp, disp_scale};
    if (reduced_args_ok("d_adcensus_stm_2s", a)) reduced_frame_device("d_adcensus_stm_2s", a, d_img_sbs, d_disp_l, d_disp_r, d_interlaced, nullptr);
}

// stm_d_adcensus_stm_2s with the history of the temporal stabilisation (stm_hip.h): stm_d_adcensus_stm_t's rules for bit 0x2000
void stm_d_adcensus_stm_2t(unsigned char *d_img_sbs, float *d_disp_l, float *d_disp_r, unsigned char *d_interlaced,
                           int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out,
                           int num_rows_disp, int num_cols_disp, int elem_sz, float disp_scale, int num_views, float angle,
                           int num_disp, int zero_disp, float ad_coeff, float census_coeff, float ucd, float lcd, int usd,
                           int lsd, int thresh_s, float thresh_h, int stages, unsigned char *d_prev_img_sbs, float *d_prev_disp_l,
                           float *d_prev_disp_r, float alpha, int thresh_color, float thresh_disp)
{
    const char *fn = "d_adcensus_stm_2t";
    const FrameArgs a = {STM_FRAME_PARAMS, stages, num_rows_disp, num_cols_disp, disp_scale};
    if (!reduced_args_ok(fn, a, true)) return;
    const TemporalHist hist = {d_prev_img_sbs, d_prev_disp_l, d_prev_disp_r, alpha, thresh_color, thresh_disp};
    bool run = false;
    if (!frame_history_ok(fn, a, hist, d_disp_l, d_disp_r, nullptr, &run)) return;
    reduced_frame_device(fn, a, d_img_sbs, d_disp_l, d_disp_r, d_interlaced, run ? &hist : nullptr);
}

// stm_d_adcensus_stm_2t on an NV12 frame (stm_hip.h): stm_d_adcensus_stm_nv12's rules, the conversion fused into the front kernel
void stm_d_adcensus_stm_2nv12(unsigned char *d_y, int pitch_y, unsigned char *d_uv, int pitch_uv, int matrix, float *d_disp_l, float *d_disp_r,
                              unsigned char *d_interlaced, int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out,
                              int num_rows_disp, int num_cols_disp, int elem_sz, float disp_scale, int num_views, float angle, int num_disp,
                              int zero_disp, float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd, int thresh_s,
                              float thresh_h, int stages, unsigned char *d_prev_img_l, unsigned char *d_prev_img_r, float *d_prev_disp_l,
                              float *d_prev_disp_r, float alpha, int thresh_color, float thresh_disp, unsigned char *d_img_l,
                              unsigned char *d_img_r)
{
    const char *fn = "d_adcensus_stm_2nv12";
    const FrameArgs a = {STM_FRAME_PARAMS, stages, num_rows_disp, num_cols_disp, disp_scale};
    if (!reduced_args_ok(fn, a, true)) return;
    if (!nv12_args_ok(fn, num_rows, num_cols_sbs, num_cols, "num_cols", pitch_y, pitch_uv, matrix)) return;
    const Nv12Input nv = {d_y, d_uv, pitch_y, pitch_uv, matrix, d_img_l, d_img_r};
    const TemporalHist hist = {nullptr, d_prev_disp_l, d_prev_disp_r, alpha, thresh_color, thresh_disp, d_prev_img_l, d_prev_img_r};
    bool run = false;
    if (!nv12_images_ok(fn, nv) || !frame_history_ok(fn, a, hist, d_disp_l, d_disp_r, &nv, &run)) return;
    reduced_frame_device(fn, a, nullptr, d_disp_l, d_disp_r, d_interlaced, run ? &hist : nullptr, &nv);
}

// the reduced-resolution frame's front as a stage (stm_hip.h): stm_k_front_low itself, the BGRX and wide planes in the workspace;
// num_cols_sbs < 2 * num_cols and stm_set_agg_variant(600): the chain of kernels it replaces
} // extern "C"
namespace {
bool front_low_args_ok(const char *fn, int num_rows, int num_cols_sbs, int num_cols, int num_rows_disp, int num_cols_disp, int elem_sz,
                       const void *census_l, const void *census_r)
{
    if (!args_ok(fn, {{"num_rows", num_rows, 1}, {"num_cols_sbs", num_cols_sbs, 1}, {"num_cols", num_cols, 1},
                      {"num_rows_disp", num_rows_disp, 1}, {"num_cols_disp", num_cols_disp, 1}, {"elem_sz", elem_sz, 3}}))
        return false;
    if ((census_l != nullptr) != (census_r != nullptr))
        return STM_REJECT("census_l, census_r", "%s: the two census planes must be both null or both set", fn);
    return true;
}
// inside a Workspace scope; cen_l / cen_r both null: the census words stay in the workspace
void front_low_device(u8 *img_l, u8 *img_r, u8 *low_l, u8 *low_r, uint32_t *cen_l, uint32_t *cen_r, const u8 *d_img_sbs, int num_cols_sbs,
                      const Nv12Input *nv, int H, int W, int h, int w, int elem_sz)
{
    const size_t hw = (size_t)h * w;
    uint32_t *pl[4];
    for (int i = 0; i < 4; ++i) pl[i] = Workspace::get<uint32_t>(hw);
    const bool want_census = cen_l != nullptr;
    if (!want_census) {
        cen_l = Workspace::get<uint32_t>(hw);
        cen_r = Workspace::get<uint32_t>(hw);
    }
    if (reduced_front_fused(num_cols_sbs, W)) {
        launch_front_low(img_l, img_r, low_l, low_r, pl[0], pl[1], pl[2], pl[3], cen_l, cen_r, nv ? nullptr : d_img_sbs, num_cols_sbs,
                         nv ? nv->y : nullptr, nv ? nv->pitch_y : 0, nv ? nv->uv : nullptr, nv ? nv->pitch_uv : 0, nv ? nv->matrix : 0, H, W, h, w,
                         elem_sz);
        return;
    }
    reduced_front_chain(img_l, img_r, low_l, low_r, d_img_sbs, num_cols_sbs, nv, H, W, h, w, elem_sz);
    if (!want_census) return;
    launch_pack_bgrx(low_l, pl[0], h, w, elem_sz);
    launch_pack_bgrx(low_r, pl[1], h, w, elem_sz);
    launch_census32_pair(pl[0], cen_l, pl[1], cen_r, h, w);
}
// the host flavour of both stage calls: the input already uploaded
void front_low_host(unsigned char *img_l, unsigned char *img_r, unsigned char *low_l, unsigned char *low_r, unsigned int *census_l,
                    unsigned int *census_r, const u8 *d_img_sbs, int num_cols_sbs, const Nv12Input *nv, int H, int W, int h, int w, int elem_sz)
{
    const size_t IMG = (size_t)H * W * elem_sz, hw = (size_t)h * w, LOW = hw * elem_sz;
    u8 *l = Workspace::get<u8>(IMG), *r = Workspace::get<u8>(IMG), *ll = Workspace::get<u8>(LOW), *lr = Workspace::get<u8>(LOW);
    uint32_t *cl = census_l ? Workspace::get<uint32_t>(hw) : nullptr, *cr = census_l ? Workspace::get<uint32_t>(hw) : nullptr;
    if (elem_sz > 3) { // bytes past a pixel's third come back 0, not as the workspace held them
        STM_CHECK(hipMemsetAsync(l, 0, IMG, stream()));
        STM_CHECK(hipMemsetAsync(r, 0, IMG, stream()));
        STM_CHECK(hipMemsetAsync(ll, 0, LOW, stream()));
        STM_CHECK(hipMemsetAsync(lr, 0, LOW, stream()));
    }
    front_low_device(l, r, ll, lr, cl, cr, d_img_sbs, num_cols_sbs, nv, H, W, h, w, elem_sz);
    down(img_l, l, IMG); down(img_r, r, IMG); down(low_l, ll, LOW); down(low_r, lr, LOW);
    if (census_l) {
        down(census_l, cl, hw);
        down(census_r, cr, hw);
    }
    sync();
}
} // namespace
extern "C" {

void stm_d_demux_sbs_low(unsigned char *d_img_l, unsigned char *d_img_r, unsigned char *d_low_l, unsigned char *d_low_r,
                         unsigned int *d_census_l, unsigned int *d_census_r, unsigned char *d_img_sbs, int num_rows, int num_cols_sbs,
                         int num_cols, int num_rows_disp, int num_cols_disp, int elem_sz)
{
    const char *fn = "d_demux_sbs_low";
    if (!front_low_args_ok(fn, num_rows, num_cols_sbs, num_cols, num_rows_disp, num_cols_disp, elem_sz, d_census_l, d_census_r)) return;
    Workspace::begin((size_t)num_rows_disp * num_cols_disp * 24 + 8192);
    front_low_device(d_img_l, d_img_r, d_low_l, d_low_r, d_census_l, d_census_r, d_img_sbs, num_cols_sbs, nullptr, num_rows, num_cols,
                     num_rows_disp, num_cols_disp, elem_sz);
}
void stm_demux_sbs_low(unsigned char *img_l, unsigned char *img_r, unsigned char *low_l, unsigned char *low_r, unsigned int *census_l,
                       unsigned int *census_r, unsigned char *img_sbs, int num_rows, int num_cols_sbs, int num_cols, int num_rows_disp,
                       int num_cols_disp, int elem_sz)
{
    const char *fn = "demux_sbs_low";
    if (!front_low_args_ok(fn, num_rows, num_cols_sbs, num_cols, num_rows_disp, num_cols_disp, elem_sz, census_l, census_r)) return;
    const size_t IMG = (size_t)num_rows * num_cols * elem_sz, hw = (size_t)num_rows_disp * num_cols_disp;
    const size_t in_sz = (size_t)num_rows * num_cols_sbs * elem_sz;
    Workspace::begin(2 * IMG + in_sz + hw * (2 * (size_t)elem_sz + 32) + 16384);
    u8 *d = up(img_sbs, in_sz);
    front_low_host(img_l, img_r, low_l, low_r, census_l, census_r, d, num_cols_sbs, nullptr, num_rows, num_cols, num_rows_disp, num_cols_disp,
                   elem_sz);
}
void stm_d_demux_nv12_low(unsigned char *d_img_l, unsigned char *d_img_r, unsigned char *d_low_l, unsigned char *d_low_r,
                          unsigned int *d_census_l, unsigned int *d_census_r, unsigned char *d_y, int pitch_y, unsigned char *d_uv, int pitch_uv,
                          int num_rows, int num_cols_sbs, int num_cols, int num_rows_disp, int num_cols_disp, int elem_sz, int matrix)
{
    const char *fn = "d_demux_nv12_low";
    if (!front_low_args_ok(fn, num_rows, num_cols_sbs, num_cols, num_rows_disp, num_cols_disp, elem_sz, d_census_l, d_census_r)) return;
    if (!nv12_args_ok(fn, num_rows, num_cols_sbs, num_cols, "num_cols", pitch_y, pitch_uv, matrix)) return;
    const Nv12Input nv = {d_y, d_uv, pitch_y, pitch_uv, matrix, nullptr, nullptr};
    Workspace::begin((size_t)num_rows_disp * num_cols_disp * 24 + 8192);
    front_low_device(d_img_l, d_img_r, d_low_l, d_low_r, d_census_l, d_census_r, nullptr, num_cols_sbs, &nv, num_rows, num_cols,
                     num_rows_disp, num_cols_disp, elem_sz);
}
void stm_demux_nv12_low(unsigned char *img_l, unsigned char *img_r, unsigned char *low_l, unsigned char *low_r, unsigned int *census_l,
                        unsigned int *census_r, unsigned char *y, int pitch_y, unsigned char *uv, int pitch_uv, int num_rows, int num_cols_sbs,
                        int num_cols, int num_rows_disp, int num_cols_disp, int elem_sz, int matrix)
{
    const char *fn = "demux_nv12_low";
    if (!front_low_args_ok(fn, num_rows, num_cols_sbs, num_cols, num_rows_disp, num_cols_disp, elem_sz, census_l, census_r)) return;
    if (!nv12_args_ok(fn, num_rows, num_cols_sbs, num_cols, "num_cols", pitch_y, pitch_uv, matrix)) return;
    // a plane's last row need not be a whole pitch long
    const size_t IMG = (size_t)num_rows * num_cols * elem_sz, hw = (size_t)num_rows_disp * num_cols_disp;
    const size_t uv_row = 2 * (size_t)((num_cols_sbs + 1) / 2);
    const size_t y_sz = (size_t)(num_rows - 1) * pitch_y + num_cols_sbs, uv_sz = (size_t)(num_rows / 2 - 1) * pitch_uv + uv_row;
    Workspace::begin(2 * IMG + y_sz + uv_sz + hw * (2 * (size_t)elem_sz + 32) + 16384);
    u8 *dy = up(y, y_sz), *duv = up(uv, uv_sz);
    const Nv12Input nv = {dy, duv, pitch_y, pitch_uv, matrix, nullptr, nullptr};
    front_low_host(img_l, img_r, low_l, low_r, census_l, census_r, nullptr, num_cols_sbs, &nv, num_rows, num_cols, num_rows_disp, num_cols_disp,
                   elem_sz);
}

void stm_adcensus_stm_2(unsigned char *img_sbs, float *disp_l, float *disp_r, unsigned char *interlaced, int num_rows,
                        int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out, int num_rows_disp,
                        int num_cols_disp, int elem_sz, float disp_scale, int num_views, float angle, int num_disp,
                        int zero_disp, float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd,
                        int thresh_s, float thresh_h)
{
    const FrameArgs a = {STM_FRAME_PARAMS, 3, num_rows_disp, num_cols_disp, disp_scale};
    frame_host("adcensus_stm_2", a, true, img_sbs, disp_l, disp_r, interlaced);
}
void stm_adcensus_stm_2s(unsigned char *img_sbs, float *disp_l, float *disp_r, unsigned char *interlaced, int num_rows,
                         int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out, int num_rows_disp,
                         int num_cols_disp, int elem_sz, float disp_scale, int num_views, float angle, int num_disp,
                         int zero_disp, float ad_coeff, float census_coeff, float ucd, float lcd, int usd, int lsd,
                         int thresh_s, float thresh_h, int stages)
{
    const FrameArgs a = {STM_FRAME_PARAMS, stages, num_rows_disp, num_cols_disp, disp_scale};
    frame_host("adcensus_stm_2s", a, true, img_sbs, disp_l, disp_r, interlaced);
}

// d_tx_scale.h:17-18  d_tx_scale (d_tx_scale.cu:83-121): despite the d_ prefix it takes HOST pointers
void stm_d_tx_scale(unsigned char *img_in, unsigned char *img_out, int in_rows, int in_cols, int out_rows, int out_cols,
                    int elem_sz)
{
    if (!args_ok("d_tx_scale", {{"in_rows", in_rows, 1}, {"in_cols", in_cols, 1}, {"out_rows", out_rows, 1},
                                {"out_cols", out_cols, 1}, {"elem_sz", elem_sz, 3}}))
        return;
    size_t in_sz = (size_t)in_rows * in_cols * elem_sz, out_sz = (size_t)out_rows * out_cols * elem_sz;
    Workspace::begin(in_sz + out_sz + 4096);
    u8 *di = up(img_in, in_sz), *dout = Workspace::get<u8>(out_sz);
    // the reference copies back an uncleared allocation (d_tx_scale.cu:95,115); here bytes past a pixel's third come back 0
    STM_CHECK(hipMemsetAsync(dout, 0, out_sz, stream()));
    launch_scale_bilinear(di, dout, in_rows, in_cols, out_rows, out_cols, elem_sz);
    down(img_out, dout, out_sz);
    sync();
}

void stm_generate_gaussian_kernel(float *kernel, int radius, float sigma)
{
    if (!args_ok("generate_gaussian_kernel", {{"radius", radius, 0}})) return;
    gaussian_kernel_2d(kernel, radius, sigma);
}

void stm_adcensus_stm(unsigned char *img_sbs, float *disp_l, float *disp_r, unsigned char *interlaced, int num_rows,
                      int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out, int elem_sz, int num_views,
                      float angle, int num_disp, int zero_disp, float ad_coeff, float census_coeff, float ucd, float lcd,
                      int usd, int lsd, int thresh_s, float thresh_h)
{
    const FrameArgs a = {STM_FRAME_PARAMS, 3};
    frame_host("adcensus_stm", a, false, img_sbs, disp_l, disp_r, interlaced);
}

} // extern "C"
