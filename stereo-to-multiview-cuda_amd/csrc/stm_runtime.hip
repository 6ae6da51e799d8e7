// stm_runtime.hip -- error policy, current stream, cached workspace, event profiler,
// host-built lookup tables.  Replaces cuda_utils.h (reference) for the HIP build.
#include "stm_common.h"
#include "../../include/stm_hip.h"

#include <float.h>
#include <math.h>
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <string>
#include <vector>

namespace stm {

// ------------------------------------------------------------------ errors
static int g_error_mode = 0;
static thread_local std::string g_last_error;
static thread_local bool g_failed = false;
bool failed() { return g_failed; }
void clear_failed() { g_failed = false; }
// Entry points nest (the host flavour of a frame call and stm_stream_submit call the device flavour after their own copies):
// only the OUTERMOST one may clear the sticky flag, or a failed upload would be forgotten by the nested call's argument screen.
static thread_local int g_api_depth = 0;
ApiNest::ApiNest() { ++g_api_depth; }
ApiNest::~ApiNest() { --g_api_depth; }
bool api_outermost() { return g_api_depth == 0; }

void fail(const char *what, const char *expr, const char *file, int line)
{
    if (g_failed && g_error_mode != 0) return; // the first error of an API call is the cause; the rest are its echoes
    char buf[1024];
    snprintf(buf, sizeof buf, "HIP error at: %s:%d\n%s %s", file, line, what, expr);
    g_last_error = buf;
    g_failed = true;
    fprintf(stderr, "%s\n", buf);
    if (g_error_mode == 0)
        exit(1); // cuda_utils.h:15-20
}
bool reject(const char *file, int line, const char *arg, const char *fmt, ...)
{
    char msg[512]; // the longest message of any screen stays below 300 bytes; vsnprintf cuts a longer one short
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    fail(msg, arg, file, line);
    return false;
}
bool ptrs_ok(const char *fn, std::initializer_list<NamedPtr> ptrs)
{
    bool ok = true;
    std::string all, list;
    size_t k = 0;
    for (const NamedPtr &p : ptrs) {
        ok = ok && p.p != nullptr;
        all += (k == 0 ? "" : k + 1 == ptrs.size() ? " and " : ", ") + std::string(p.name);
        list += (k++ == 0 ? "" : ", ") + std::string(p.name);
    }
    return ok || STM_REJECT(list.c_str(), "%s: %s must not be null", fn, all.c_str());
}

// ------------------------------------------------------------------ stream
static thread_local hipStream_t g_stream = nullptr;
hipStream_t stream() { return g_stream; }

// ------------------------------------------------------------------ device-side diagnostics
static std::mutex g_diag_mu;
static uint32_t *g_diag[64] = {nullptr};
uint32_t *device_diag()
{
    int dev = 0;
    STM_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) {
        fail("device index out of range", "hipGetDevice", __FILE__, __LINE__);
        return nullptr;
    }
    std::lock_guard<std::mutex> lock(g_diag_mu);
    if (!g_diag[dev]) {
        STM_CHECK(hipMalloc((void **)&g_diag[dev], 64));
        STM_CHECK(hipMemset(g_diag[dev], 0, 64));
    }
    return g_diag[dev];
}
// reads and clears the current device's word (after the current stream has drained); 0 when it was never allocated
static uint32_t take_device_diag()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    uint32_t *p;
    {
        std::lock_guard<std::mutex> lock(g_diag_mu);
        p = g_diag[dev];
    }
    if (!p) return 0;
    uint32_t v = 0;
    if (hipStreamSynchronize(g_stream) != hipSuccess) return 0;
    if (hipMemcpy(&v, p, 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    if (v) (void)hipMemset(p, 0, 4);
    return v;
}

// --------------------------------------------------------------- workspace
// one slab per host thread and device (two threads may drive the same GPU on their own streams); grows
// geometrically, never shrinks until the owning thread calls stm_release_workspace
struct WsState {
    char *base = nullptr;
    size_t cap = 0;
    size_t off = 0;
    std::vector<void *> retired; // old slabs still possibly referenced by in-flight kernels
};
constexpr int WS_DEVS = 64; // one shared slab per device and thread (the same bound as the host-frame staging buffers)
static thread_local WsState g_ws[WS_DEVS];

static thread_local WsState *g_ws_bound = nullptr; // a private workspace bound by a frame stream (see below)

static WsState &ws()
{
    if (g_ws_bound) return *g_ws_bound;
    int dev = 0;
    STM_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= WS_DEVS) { // two devices must never share a slab: refuse instead of aliasing
        fail("workspace: device index out of range", "hipGetDevice", __FILE__, __LINE__);
        dev = 0; // only reached in error mode 1: the failed() flag keeps alloc() from handing anything out
    }
    return g_ws[dev];
}

// A private workspace for an object that replays captured work (stm_stream's hipGraph): its addresses must not move
// when some other call on the same thread grows the shared slab.
void *ws_private_create() { return new WsState(); }
void ws_private_bind(void *p) { g_ws_bound = (WsState *)p; }
void ws_private_destroy(void *p)
{
    WsState *w = (WsState *)p;
    if (!w) return;
    if (g_ws_bound == w) g_ws_bound = nullptr;
    STM_CHECK(hipDeviceSynchronize());
    for (void *q : w->retired) STM_CHECK(hipFree(q));
    if (w->base) STM_CHECK(hipFree(w->base));
    delete w;
}
// base address and capacity of the workspace in use: lets a caller notice that a replayed capture went stale
void ws_identity(void **base, size_t *cap)
{
    WsState &w = ws();
    *base = w.base;
    *cap = w.cap;
}

void Workspace::begin(size_t hint)
{
    WsState &w = ws();
    w.off = 0;
    if (failed()) return;
    if (hint > w.cap) {
        // grow before carving so that one scope never straddles two slabs
        if (w.base) {
            STM_CHECK(hipStreamSynchronize(stream()));
            STM_CHECK(hipFree(w.base));
            w.base = nullptr;
            w.cap = 0;
        }
        size_t cap = hint + (hint >> 3) + (1u << 20);
        char *nb = nullptr;
        if (hipMalloc((void **)&nb, cap) != hipSuccess || !nb) { // commit base / cap only after success
            (void)hipGetLastError();
            fail("workspace allocation failed", "hipMalloc", __FILE__, __LINE__);
            return;
        }
        w.base = nb;
        w.cap = cap;
    }
}

// After a failure (error mode 1) every request is answered from a small static host buffer that no kernel will ever see:
// launches are suppressed (STM_LAUNCH) and the copy calls that might receive it fail cleanly instead of faulting.
void *Workspace::alloc(size_t bytes)
{
    static char sink[256];
    WsState &w = ws();
    if (failed()) return sink;
    size_t a = (w.off + 255) & ~(size_t)255;
    if (a + bytes > w.cap) {
        // Late growth: earlier carve-outs of this scope live in the old slab and kernels
        // may be in flight on them, so retire (do not free) it until release.
        size_t cap = (a + bytes) * 2 + (1u << 20);
        char *nb = nullptr;
        if (hipMalloc((void **)&nb, cap) != hipSuccess || !nb) {
            (void)hipGetLastError();
            fail("workspace allocation failed", "hipMalloc", __FILE__, __LINE__);
            return sink;
        }
        if (w.base) w.retired.push_back(w.base);
        w.base = nb;
        w.cap = cap;
        a = 0;
    }
    w.off = a + bytes;
    return w.base + a;
}

static void ws_release()
{
    WsState &w = ws();
    STM_CHECK(hipDeviceSynchronize());
    for (void *p : w.retired) STM_CHECK(hipFree(p));
    w.retired.clear();
    if (w.base) STM_CHECK(hipFree(w.base));
    w.base = nullptr;
    w.cap = w.off = 0;
}

// ---------------------------------------------------------------- profiler
struct ProfRec {
    std::string name;
    hipEvent_t a, b;
};
static int g_prof_on = 0; // 0 off, 1 every named kernel, 2 the aggregation kernels only (a few events per frame)
bool prof_enabled() { return g_prof_on != 0; }
static std::vector<ProfRec> g_prof;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_pool;
static std::mutex g_prof_mu; // host threads may drive the library concurrently (stm_hip.h)

ProfScope::ProfScope(const char *name) : slot(-1)
{
    if (!g_prof_on) return;
    if (g_prof_on == 2 && strncmp(name, "pq_", 3) != 0 && strncmp(name, "agg_", 4) != 0 && strcmp(name, "cost_init") != 0) return;
    ProfRec r;
    r.name = name;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (!g_prof_pool.empty()) {
        r.a = g_prof_pool.back().first;
        r.b = g_prof_pool.back().second;
        g_prof_pool.pop_back();
    } else {
        STM_CHECK(hipEventCreate(&r.a));
        STM_CHECK(hipEventCreate(&r.b));
    }
    STM_CHECK(hipEventRecord(r.a, stream()));
    slot = (int)g_prof.size();
    g_prof.push_back(r);
    ev_b = r.b;
}
ProfScope::~ProfScope()
{
    if (slot >= 0) STM_CHECK(hipEventRecord((hipEvent_t)ev_b, stream()));
}

static int g_agg_variant = 0;
int agg_variant() { return g_agg_variant; }
static int g_ref_quirks = 0;
int ref_quirks() { return g_ref_quirks; }
static int g_irv_paper_ratio = 0;
int irv_paper_ratio() { return g_irv_paper_ratio; }
static int g_irv_chunk = 0;
int irv_chunk() { return g_irv_chunk; }
// the calling thread's display geometry (stm_set_lens)
static thread_local Lens g_lens = {0, 0.0, 0.0, 0.0};
Lens lens() { return g_lens; }
void set_lens(const Lens &l) { g_lens = l; }
bool lens_params_ok(const char *fn, int mode, int mode_lo, int mode_hi, double pitch, double slope, double centre)
{
    if (mode < mode_lo || mode > mode_hi) return STM_REJECT("mode", "%s: lens mode = %d, must be in %d .. %d", fn, mode, mode_lo, mode_hi);
    if (mode == 0) return true; // off: the other arguments are ignored
    if (!(pitch >= 1.0) || std::isinf(pitch)) // NaN fails the comparison
        return STM_REJECT("pitch", "%s: lens pitch = %g, must be finite and >= 1 (sub-pixels per lens)", fn, pitch);
    if (!std::isfinite(slope)) return STM_REJECT("slope", "%s: lens slope = %g, must be finite", fn, slope);
    if (!std::isfinite(centre)) return STM_REJECT("centre", "%s: lens centre = %g, must be finite", fn, centre);
    return true;
}

// the calling thread's output geometry (stm_set_layout)
static thread_local Layout g_layout = {0, 1, 1, 0, 0};
Layout layout() { return g_layout; }
void set_layout(const Layout &l) { g_layout = l; }
bool layout_params_ok(const char *fn, int layout, int tiles_x, int tiles_y, int order, int filter)
{
    if (layout != 0 && layout != 1) return STM_REJECT("layout", "%s: layout = %d, must be 0 (interlaced) or 1 (quilt)", fn, layout);
    if (layout == 0) return true; // interlaced: the other arguments are ignored
    if (tiles_x < 1 || tiles_x > 65535) return STM_REJECT("tiles_x", "%s: tiles_x = %d, must be in 1 .. 65535", fn, tiles_x);
    if (tiles_y < 1 || tiles_y > 65535) return STM_REJECT("tiles_y", "%s: tiles_y = %d, must be in 1 .. 65535", fn, tiles_y);
    if (order < 0 || order > 3)
        return STM_REJECT("order", "%s: order = %d, must be 0 .. 3 (bit 0: tile rows bottom-up, bit 1: view order reversed)", fn, order);
    if (filter != 0 && filter != 1)
        return STM_REJECT("filter", "%s: filter = %d, must be 0 (four-neighbour sampler) or 1 (area average)", fn, filter);
    return true;
}
// the calling thread's output format (stm_set_output)
static thread_local Output g_output = {0, 0, 0, 0};
Output output() { return g_output; }
void set_output(const Output &o) { g_output = o; }
bool output_params_ok(const char *fn, int format, int matrix, int pitch, int uv_row)
{
    if (format != 0 && format != 1) return STM_REJECT("format", "%s: format = %d, must be 0 (BGR) or 1 (NV12)", fn, format);
    if (format == 0) return true; // BGR: the other arguments are ignored
    if (matrix < 0 || matrix > 3)
        return STM_REJECT("matrix", "%s: matrix = %d, must be 0 (BT.601 limited), 1 (BT.709 limited), 2 (BT.601 full) or 3 (BT.709 full)", fn, matrix);
    if (pitch < 0) return STM_REJECT("pitch", "%s: pitch = %d, must be >= 0 (0: num_cols_out)", fn, pitch);
    if (uv_row < 0) return STM_REJECT("uv_row", "%s: uv_row = %d, must be >= 0 (0: num_rows_out)", fn, uv_row);
    return true;
}
// the calling thread's overlay (stm_set_overlay)
static thread_local Overlay g_overlay = {0, nullptr, 0, 0, 0, 0, 0.0f};
Overlay overlay() { return g_overlay; }
void set_overlay(const Overlay &o) { g_overlay = o; }
bool overlay_params_ok(const char *fn, const void *ov, bool check_ptr, int ov_rows, int ov_cols, int x0, int y0, float disparity)
{
    if (check_ptr && !ov) return STM_REJECT("overlay", "%s: the overlay is null", fn);
    if (check_ptr && ((uintptr_t)ov & 3) != 0)
        return STM_REJECT("overlay", "%s: the overlay must be 4-byte aligned (a pixel is read as one word)", fn);
    if (ov_rows < 1 || ov_rows > 65535) return STM_REJECT("ov_rows", "%s: ov_rows = %d, must be in 1 .. 65535", fn, ov_rows);
    if (ov_cols < 1 || ov_cols > 65535) return STM_REJECT("ov_cols", "%s: ov_cols = %d, must be in 1 .. 65535", fn, ov_cols);
    if (x0 < -65536 || x0 > 65536) return STM_REJECT("x0", "%s: x0 = %d, must be in -65536 .. 65536", fn, x0);
    if (y0 < -65536 || y0 > 65536) return STM_REJECT("y0", "%s: y0 = %d, must be in -65536 .. 65536", fn, y0);
    if (!(fabsf(disparity) <= 4096.0f)) // NaN fails the comparison
        return STM_REJECT("disparity", "%s: disparity = %g, must be finite and of magnitude <= 4096", fn, (double)disparity);
    return true;
}
// the calling thread's test tap on the aggregation chain (stm_set_agg_tap)
static thread_local AggTap g_agg_tap = {nullptr, nullptr, nullptr, nullptr};
AggTap agg_tap() { return g_agg_tap; }
void set_agg_tap(const AggTap &t) { g_agg_tap = t; }
// the calling thread's test tap on the scanline passes (stm_set_hslo_tap)
static thread_local HsloTap g_hslo_tap = {nullptr, nullptr, nullptr};
HsloTap hslo_tap() { return g_hslo_tap; }
void set_hslo_tap(const HsloTap &t) { g_hslo_tap = t; }
// the calling thread's automatic overlay placement (stm_set_overlay_auto)
OverlayAuto overlay_auto_default() { return OverlayAuto{0, 20, 1.0f, 8, 0.0f, 0.0f, 1.0f, 0.1f, nullptr}; }
static thread_local OverlayAuto g_overlay_auto = overlay_auto_default();
OverlayAuto overlay_auto() { return g_overlay_auto; }
void set_overlay_auto(const OverlayAuto &a) { g_overlay_auto = a; }
bool overlay_auto_params_ok(const char *fn, int near_permille, float margin, int pad, float limit_lo, float limit_hi, float rate_near,
                            float rate_far)
{
    if (near_permille < 0 || near_permille > 499)
        return STM_REJECT("near_permille", "%s: near_permille = %d, must be in 0 .. 499", fn, near_permille);
    if (!(fabsf(margin) <= 4096.0f)) // NaN fails the comparison
        return STM_REJECT("margin", "%s: margin = %g, must be finite and of magnitude <= 4096", fn, (double)margin);
    if (pad < 0 || pad > 4096) return STM_REJECT("pad", "%s: pad = %d, must be in 0 .. 4096", fn, pad);
    if (!(fabsf(limit_lo) <= 4096.0f))
        return STM_REJECT("limit_lo", "%s: limit_lo = %g, must be finite and of magnitude <= 4096", fn, (double)limit_lo);
    if (!(fabsf(limit_hi) <= 4096.0f))
        return STM_REJECT("limit_hi", "%s: limit_hi = %g, must be finite and of magnitude <= 4096", fn, (double)limit_hi);
    if (!(limit_lo <= limit_hi))
        return STM_REJECT("limit_lo, limit_hi", "%s: limit_lo = %g > limit_hi = %g", fn, (double)limit_lo, (double)limit_hi);
    if (!(rate_near > 0.0f && rate_near <= 1.0f)) return STM_REJECT("rate_near", "%s: rate_near = %g, must be in (0, 1]", fn, (double)rate_near);
    if (!(rate_far > 0.0f && rate_far <= 1.0f)) return STM_REJECT("rate_far", "%s: rate_far = %g, must be in (0, 1]", fn, (double)rate_far);
    return true;
}
bool overlay_fit_size_ok(const char *fn, int num_rows, int num_cols)
{
    if ((size_t)num_rows * num_cols <= 0x7fffffffu) return true;
    return STM_REJECT("num_rows, num_cols", "%s: num_rows * num_cols = %zu, must be below 2^31 (the overlay's fit counts in 32 bits)", fn,
                      (size_t)num_rows * num_cols);
}
// stm_mux_nv12's coefficients (stm_hip.h): each rounded one computed in double and rounded to nearest, the three derived ones by
// subtraction, so that white lands on the range's end and every grey on 128 / 128
Nv12OutCoef nv12_out_coef(int matrix)
{
    const double Kr = (matrix & 1) ? 0.2126 : 0.299, Kb = (matrix & 1) ? 0.0722 : 0.114;
    const bool full = matrix >= 2;
    const double sy = full ? 1.0 : 219.0 / 255.0, sc = full ? 1.0 : 224.0 / 255.0;
    Nv12OutCoef k;
    k.yo = full ? 0 : 16;
    const int ys = (int)std::lround(65536.0 * sy);
    k.yr = (int)std::lround(65536.0 * Kr * sy);
    k.yb = (int)std::lround(65536.0 * Kb * sy);
    k.yg = ys - k.yr - k.yb;
    k.h = (int)std::lround(32768.0 * sc);
    k.ur = (int)std::lround(65536.0 * Kr * sc / (2.0 * (1.0 - Kb)));
    k.ug = k.h - k.ur;
    k.vb = (int)std::lround(65536.0 * Kb * sc / (2.0 * (1.0 - Kr)));
    k.vg = k.h - k.vb;
    return k;
}
Nv12Out nv12_out(u8 *y, size_t pitch_y, u8 *uv, size_t pitch_uv, int matrix)
{
    const int pairs = (((uintptr_t)y | (uintptr_t)uv | pitch_y | pitch_uv) & 1) == 0;
    return Nv12Out{y, uv, pitch_y, pitch_uv, nv12_out_coef(matrix), pairs};
}
Nv12Out nv12_out_surface(u8 *surface, const Output &o, int Hout, int Wout)
{
    const size_t P = o.pitch ? o.pitch : Wout, R = o.uv_row ? o.uv_row : Hout;
    return nv12_out(surface, P, surface + P * R, P, o.matrix);
}
size_t frame_out_bytes(int Hout, int Wout, int elem_sz)
{
    const Output o = output();
    if (o.format == 0) return (size_t)Hout * Wout * elem_sz;
    const size_t P = o.pitch ? o.pitch : Wout, R = o.uv_row ? o.uv_row : Hout;
    return P * (R + (size_t)Hout / 2);
}
static int g_quilt_lds_limit = 32 * 1024; // five workgroups of the staged kernel share a CU's 160 KiB
int quilt_lds_limit() { return g_quilt_lds_limit; }

// the calling thread's input packing (stm_set_packing)
static thread_local Packing g_packing = {0, 0, 0, 0};
Packing packing() { return g_packing; }
void set_packing(const Packing &p) { g_packing = p; }
bool packing_params_ok(const char *fn, const Packing &pk)
{
    if (pk.packing < 0 || pk.packing > 3)
        return STM_REJECT("packing", "%s: packing = %d, must be 0 (side by side), 1 (half-width side by side), 2 (top and bottom) or 3 (half-height top and bottom)", fn, pk.packing);
    if (pk.swap != 0 && pk.swap != 1) return STM_REJECT("swap", "%s: swap = %d, must be 0 (left eye first) or 1 (right eye first)", fn, pk.swap);
    if (pk.filter != 0 && pk.filter != 1) return STM_REJECT("filter", "%s: filter = %d, must be 0 (linear) or 1 (Catmull-Rom)", fn, pk.filter);
    if (pk.gap < 0 || pk.gap > (1 << 24)) return STM_REJECT("gap", "%s: gap = %d, must be >= 0 (and at most 2^24)", fn, pk.gap);
    if (pk.filter != 0 && (pk.packing & 1) == 0)
        return STM_REJECT("filter", "%s: filter = %d with packing = %d: a full packing copies, the filter must be 0", fn, pk.filter, pk.packing);
    return true;
}

// the calling thread's depth budget (stm_set_depth, stm_set_depth_auto)
static thread_local Depth g_depth = {0, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 20, nullptr}; // disp_lo == disp_hi: no budget set yet
Depth depth() { return g_depth; }
void set_depth(const Depth &d) { g_depth = d; }
bool depth_params_ok(const char *fn, int mode, float gain, float conv)
{
    if (mode < 0 || mode > 2) return STM_REJECT("mode", "%s: depth mode = %d, must be 0 (off), 1 (manual) or 2 (automatic)", fn, mode);
    if (mode != 1) return true; // off / automatic: gain and conv are ignored
    if (!(gain >= 0.0f && gain <= 8.0f)) // NaN fails the comparison
        return STM_REJECT("gain", "%s: depth gain = %g, must be in [0, 8]", fn, (double)gain);
    if (!(fabsf(conv) <= 4096.0f)) return STM_REJECT("conv", "%s: depth conv = %g, must be finite with |conv| <= 4096", fn, (double)conv);
    return true;
}
// the calling thread's view antialiasing (stm_set_antialias)
static thread_local Antialias g_antialias = {0, 0.0f, 0, 0.0f};
Antialias antialias() { return g_antialias; }
void set_antialias(const Antialias &a) { g_antialias = a; }
bool antialias_params_ok(const char *fn, float strength, int max_radius, float gate)
{
    if (!(strength >= 0.0f && strength <= 8.0f)) // NaN fails the comparison
        return STM_REJECT("strength", "%s: antialias strength = %g, must be in [0, 8]", fn, (double)strength);
    if (max_radius < 1 || max_radius > 16) return STM_REJECT("max_radius", "%s: antialias max_radius = %d, must be in 1 .. 16", fn, max_radius);
    if (!(gate >= 0.0f && gate <= FLT_MAX)) return STM_REJECT("gate", "%s: antialias gate = %g, must be finite and >= 0", fn, (double)gate);
    return true;
}
// the calling thread's vertical alignment (stm_set_align, stm_set_align_auto)
static thread_local Align g_align = {0, 0.0f, 0.0f, 0.0f, 16, 1.0f, nullptr};
Align align() { return g_align; }
void set_align(const Align &a) { g_align = a; }
bool align_params_ok(const char *fn, int mode, float a, float b, float c)
{
    if (mode < 0 || mode > 2) return STM_REJECT("mode", "%s: align mode = %d, must be 0 (off), 1 (manual) or 2 (automatic)", fn, mode);
    if (mode != 1) return true; // off / automatic: a, b and c are ignored
    if (!(fabsf(a) <= FLT_MAX)) return STM_REJECT("a", "%s: align a = %g, must be finite", fn, (double)a); // NaN fails the comparison
    if (!(fabsf(b) <= FLT_MAX)) return STM_REJECT("b", "%s: align b = %g, must be finite", fn, (double)b);
    if (!(fabsf(c) <= FLT_MAX)) return STM_REJECT("c", "%s: align c = %g, must be finite", fn, (double)c);
    return true;
}
// the calling thread's rectification: installed by a frame stream only (stm_stream_rectify), there is no exported setter
static thread_local Rectify g_rectify = {0, {{0.0f}, {0.0f}}, 0};
Rectify rectify() { return g_rectify; }
void set_rectify(const Rectify &r) { g_rectify = r; }
bool rectify_params_ok(const char *fn, const float *rec18, int border)
{
    if (border != 0 && border != 1) return STM_REJECT("border", "%s: border = %d, must be 0 (taps outside are 0) or 1 (clamped)", fn, border);
    for (int i = 0; i < 18; ++i)
        if (!(fabsf(rec18[i]) <= FLT_MAX)) // NaN fails the comparison
            return STM_REJECT("rec18", "%s: rec18[%d] = %g, must be finite", fn, i, (double)rec18[i]);
    return true;
}
bool align_auto_params_ok(const char *fn, int radius, float rate)
{
    if (radius < 1 || radius > 32) return STM_REJECT("radius", "%s: radius = %d, must be in 1 .. 32", fn, radius);
    if (!(rate > 0.0f && rate <= 1.0f)) return STM_REJECT("rate", "%s: rate = %g, must be in (0, 1]", fn, (double)rate);
    return true;
}
bool align_size_ok(const char *fn, int num_rows, int num_cols)
{
    if (num_rows < 4 || num_cols < 8)
        return STM_REJECT("num_rows, num_cols", "%s: the alignment measurement needs num_rows >= 4 and num_cols >= 8 (got %d x %d)", fn, num_rows,
                          num_cols);
    // a block's sum of |G_L - G_R| is at most 510 (W/8 + 1) (H/4 + 1), kept in 32 bits
    if ((unsigned long long)(num_rows / 4 + 1) * (unsigned long long)(num_cols / 8 + 1) > 0xffffffffull / 510)
        return STM_REJECT("num_rows, num_cols", "%s: the alignment measurement needs (num_rows/4 + 1) * (num_cols/8 + 1) <= %llu (got %d x %d)", fn,
                          0xffffffffull / 510, num_rows, num_cols);
    return true;
}
// the calling thread's colour balance (stm_set_balance, stm_set_balance_auto)
Balance balance_default()
{
    Balance b;
    b.mode = 0;
    for (int i = 0; i < 768; ++i) b.lut[i] = (u8)i;
    b.max_shift = 48;
    b.rate = 1.0f;
    b.d_state = nullptr;
    return b;
}
static thread_local Balance g_balance = balance_default();
Balance balance() { return g_balance; }
void set_balance(const Balance &b) { g_balance = b; }
bool balance_params_ok(const char *fn, int mode, const u8 *lut768)
{
    if (mode < 0 || mode > 2) return STM_REJECT("mode", "%s: balance mode = %d, must be 0 (off), 1 (given) or 2 (measured)", fn, mode);
    if (mode == 1 && !lut768) return STM_REJECT("lut768", "%s: lut768 must not be null in mode 1", fn); // off / measured: lut768 is ignored
    return true;
}
bool balance_auto_params_ok(const char *fn, int max_shift, float rate)
{
    if (max_shift < 0 || max_shift > 255) return STM_REJECT("max_shift", "%s: max_shift = %d, must be in 0 .. 255", fn, max_shift);
    if (!(rate > 0.0f && rate <= 1.0f)) return STM_REJECT("rate", "%s: rate = %g, must be in (0, 1]", fn, (double)rate); // NaN fails the comparison
    return true;
}
bool balance_size_ok(const char *fn, int num_rows, int num_cols)
{
    if ((long long)num_rows * (long long)num_cols < (1ll << 31)) return true;
    return STM_REJECT("num_rows, num_cols", "%s: the balance measurement needs num_rows * num_cols < 2147483648 (got %d x %d)", fn, num_rows, num_cols);
}
int balance_rate_q(float rate)
{
    const int q = (int)floorf(rate * 256.0f + 0.5f);
    return q < 1 ? 1 : q > 256 ? 256 : q;
}
// the calling thread's shot-change detector (stm_set_cut)
Cut cut_default() { return Cut{0, CUT_DEFAULT_THRESH, 1, nullptr}; }
static thread_local Cut g_cut = cut_default();
Cut cut() { return g_cut; }
void set_cut(const Cut &c) { g_cut = c; }
bool cut_params_ok(const char *fn, int thresh_permille, int min_gap)
{
    if (thresh_permille < 1 || thresh_permille > 1000)
        return STM_REJECT("thresh_permille", "%s: thresh_permille = %d, must be in 1 .. 1000", fn, thresh_permille);
    if (min_gap < 1 || min_gap > (1 << 20)) return STM_REJECT("min_gap", "%s: min_gap = %d, must be in 1 .. 1048576", fn, min_gap);
    return true;
}
bool cut_size_ok(const char *fn, int num_rows, int num_cols)
{
    if (num_rows >= 4 && num_cols >= 4 && (long long)num_rows * (long long)num_cols < (1ll << 31)) return true;
    return STM_REJECT("num_rows, num_cols",
                      "%s: the shot-change detector needs num_rows, num_cols >= 4 and num_rows * num_cols < 2147483648 (got %d x %d)", fn, num_rows,
                      num_cols);
}
// the calling thread's active picture area (stm_set_active, stm_set_active_auto)
Active active_default() { return Active{0, {0, 0, 0, 0}, 0, 0.0f, 24, 10, 300, 12, nullptr}; }
static thread_local Active g_active = active_default();
Active active() { return g_active; }
void set_active(const Active &a) { g_active = a; }
bool active_params_ok(const char *fn, int mode, const int *rect, int fill, float fill_disp)
{
    if (mode < 0 || mode > 2) return STM_REJECT("mode", "%s: active mode = %d, must be 0 (off), 1 (given) or 2 (measured)", fn, mode);
    if (mode == 0) return true; // off: the other arguments are ignored
    if (mode == 1 && !rect) return STM_REJECT("rect", "%s: rect must not be null in mode 1", fn);
    if (mode == 1 && !(rect[0] >= 0 && rect[0] < rect[1] && rect[2] >= 0 && rect[2] < rect[3]))
        return STM_REJECT("rect", "%s: rect = {%d, %d, %d, %d}, must hold 0 <= top < bottom and 0 <= left < right", fn, rect[0], rect[1], rect[2],
                          rect[3]);
    if (fill != 0 && fill != 1) return STM_REJECT("fill", "%s: fill = %d, must be 0 or 1", fn, fill);
    if (!(fabsf(fill_disp) <= 4096.0f)) // NaN fails the comparison
        return STM_REJECT("fill_disp", "%s: fill_disp = %g, must be finite and of magnitude <= 4096", fn, (double)fill_disp);
    return true;
}
bool active_auto_params_ok(const char *fn, int thresh_luma, int lit_permille, int max_bar_permille, int hold)
{
    if (thresh_luma < 0 || thresh_luma > 254) return STM_REJECT("thresh_luma", "%s: thresh_luma = %d, must be in 0 .. 254", fn, thresh_luma);
    if (lit_permille < 0 || lit_permille > 999) return STM_REJECT("lit_permille", "%s: lit_permille = %d, must be in 0 .. 999", fn, lit_permille);
    if (max_bar_permille < 0 || max_bar_permille > 450)
        return STM_REJECT("max_bar_permille", "%s: max_bar_permille = %d, must be in 0 .. 450", fn, max_bar_permille);
    if (hold < 1 || hold > (1 << 20)) return STM_REJECT("hold", "%s: hold = %d, must be in 1 .. 1048576", fn, hold);
    return true;
}
bool active_size_ok(const char *fn, int num_rows, int num_cols)
{
    if ((long long)num_rows * (long long)num_cols < (1ll << 31)) return true;
    return STM_REJECT("num_rows, num_cols", "%s: the active area needs num_rows * num_cols < 2147483648 (got %d x %d)", fn, num_rows, num_cols);
}
bool active_rect_ok(const char *fn, const int *rect, int num_rows, int num_cols)
{
    if (rect[0] >= 0 && rect[0] < rect[1] && rect[1] <= num_rows && rect[2] >= 0 && rect[2] < rect[3] && rect[3] <= num_cols) return true;
    return STM_REJECT("rect", "%s: the active rectangle {%d, %d, %d, %d} must hold 0 <= top < bottom <= num_rows = %d and 0 <= left < right <= "
                      "num_cols = %d", fn, rect[0], rect[1], rect[2], rect[3], num_rows, num_cols);
}
bool depth_auto_params_ok(const char *fn, float disp_lo, float disp_hi, float max_gain, int clip_permille, float rate)
{
    if (!(fabsf(disp_lo) <= 4096.0f) || !(fabsf(disp_hi) <= 4096.0f) || !(disp_lo < disp_hi))
        return STM_REJECT("disp_lo, disp_hi", "%s: depth budget [%g, %g]: disp_lo < disp_hi, both finite and of magnitude <= 4096", fn,
                          (double)disp_lo, (double)disp_hi);
    if (!(max_gain > 0.0f && max_gain <= 8.0f)) return STM_REJECT("max_gain", "%s: max_gain = %g, must be in (0, 8]", fn, (double)max_gain);
    if (clip_permille < 0 || clip_permille > 499) return STM_REJECT("clip_permille", "%s: clip_permille = %d, must be in 0 .. 499", fn, clip_permille);
    if (!(rate > 0.0f && rate <= 1.0f)) return STM_REJECT("rate", "%s: rate = %g, must be in (0, 1]", fn, (double)rate);
    return true;
}

// ------------------------------------------------------------------ tables
// rho(c) = 1 - exp(-c/lambda): d_ci_adcensus.cu:27-34 with inv = 1.0/coeff narrowed (:160).
// The reference's __expf is replaced by a correctly rounded exp evaluated on the host once per
// distinct input: the AD term takes only 766 values ((|dB|+|dG|+|dR|) * 0.33333334f, d_ci_ad.cu:146-157),
// the census term 65 (Hamming 0..64, d_alu.cu:7-15).  The kernels index these tables, so CPU and GPU
// cost volumes agree bit for bit (SURVEY A-Q8).
static inline float rho(float c, float inv)
{
    float t = -c * inv;
    float e = (float)exp((double)t);
    return (float)(1.0 - (double)e);
}
void rho_luts(float ad_coeff, float census_coeff, float *lut_ad, float *lut_census)
{
    float inv_ad = (float)(1.0 / (double)ad_coeff);
    float inv_c = (float)(1.0 / (double)census_coeff);
    for (int k = 0; k <= 765; ++k) lut_ad[k] = rho((float)k * 0.33333334f, inv_ad);
    for (int h = 0; h <= 64; ++h) lut_census[h] = rho((float)h, inv_c);
}
// generateGaussianKernel / gaussian2D: d_filter_gaussian.cu:237-255 (PI literal :7)
void gaussian_kernel_2d(float *kernel, int radius, float sigma)
{
    const float PI = 3.14159265359f;
    int kw = radius * 2 + 1;
    for (int y = -radius; y <= radius; ++y)
        for (int x = -radius; x <= radius; ++x) {
            float fx = (float)x, fy = (float)y;
            float variance = (float)pow((double)sigma, 2.0);
            float exponent = (float)(-(pow((double)fx, 2.0) + pow((double)fy, 2.0)) / (double)(2 * variance));
            kernel[(x + radius) + (y + radius) * kw] = expf(exponent) / (2 * PI * variance);
        }
}
// generateGaussian1D / gaussian1D_host: d_filter_bilateral.cu:26-39 (PI literal :8)
void gaussian_kernel_1d(float *kernel, int size, float sigma)
{
    const float PI = 3.14159265359f;
    for (int i = 0; i < size; ++i) {
        float x = (float)i;
        float variance = (float)pow((double)sigma, 2.0);
        float power = (float)pow((double)x, 2.0);
        float exponent = -power / (2 * variance);
        kernel[i] = expf(exponent) / sqrtf(2 * PI * variance);
    }
}
// y_interval: d_mux_multiview.cu:146 (PI literal :8)
float mux_y_interval(int num_views, float angle, int elem_sz)
{
    const float PI = 3.1415926535f;
    float a = angle * PI;
    double t = tan((double)a / 180.0);
    return (float)((double)(float)num_views / t / (double)(float)elem_sz);
}

} // namespace stm

// ------------------------------------------------------------------- C ABI
extern "C" {
int stm_version(void) { return 100; }
void stm_set_stream(void *s) { stm::g_stream = (hipStream_t)s; }
void *stm_get_stream(void) { return (void *)stm::g_stream; }
void stm_set_error_mode(int m) { stm::g_error_mode = m; }
const char *stm_last_error(void)
{
    // a clamp inside a kernel (IrvArgs::diag) becomes an error of the calling thread here; this waits for the thread's stream
    const uint32_t d = stm::take_device_diag();
    if (d) {
        char buf[256];
        snprintf(buf, sizeof buf, "dr_irv: the outlier list was inconsistent and was clamped (bits 0x%x: 1 = append past the capacity dropped, 2 = counter beyond the capacity, 4 = entry outside the frame); outliers may have been skipped", d);
        stm::g_last_error = buf;
    }
    return stm::g_last_error.c_str();
}
void stm_release_workspace(void)
{
    stm::ws_release();
    stm::release_host_frame_bufs();
}
void stm_prof_enable(int on) { stm::g_prof_on = on < 0 ? 0 : on; }
void stm_prof_reset(void)
{
    std::lock_guard<std::mutex> lock(stm::g_prof_mu);
    for (auto &r : stm::g_prof) stm::g_prof_pool.push_back({r.a, r.b});
    stm::g_prof.clear();
}
int stm_prof_read(const char *kernel, float *total_ms)
{
    int n = 0;
    float tot = 0.f;
    std::lock_guard<std::mutex> lock(stm::g_prof_mu);
    for (auto &r : stm::g_prof) {
        if (r.name != kernel) continue;
        STM_CHECK(hipEventSynchronize(r.b));
        float ms = 0.f;
        STM_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
        tot += ms;
        ++n;
    }
    if (total_ms) *total_ms = tot;
    return n;
}
void stm_set_ref_quirks(int on) { stm::g_ref_quirks = on ? 1 : 0; }
void stm_set_irv_paper_ratio(int on) { stm::g_irv_paper_ratio = on ? 1 : 0; }
int stm_set_irv_chunk(int entries)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (entries < 0 || entries > 16) // the setting stays as it was
        return STM_REJECT("entries", "set_irv_chunk: entries = %d, must be 0 (the library's own rule) or 1 .. 16", entries) ? 0 : -1;
    stm::g_irv_chunk = entries;
    return 0;
}
int stm_irv_path(int num_rows, int num_cols, int usd, int iterations, int device_flavour, int with_dcc)
{
    return stm::irv_path(num_rows, num_cols, usd, iterations, device_flavour != 0, with_dcc != 0);
}
int stm_set_lens(int mode, double pitch, double slope, double centre)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (!stm::lens_params_ok("set_lens", mode, 0, 3, pitch, slope, centre)) return -1; // the thread's geometry stays as it was
    stm::set_lens(mode == 0 ? stm::Lens{0, 0.0, 0.0, 0.0} : stm::Lens{mode, pitch, slope, centre});
    return 0;
}
int stm_set_layout(int layout, int tiles_x, int tiles_y, int order, int filter)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (!stm::layout_params_ok("set_layout", layout, tiles_x, tiles_y, order, filter)) return -1; // the thread's layout stays as it was
    stm::set_layout(layout == 0 ? stm::Layout{0, 1, 1, 0, 0} : stm::Layout{layout, tiles_x, tiles_y, order, filter});
    return 0;
}
void stm_get_layout(int *out)
{
    const stm::Layout lo = stm::layout();
    out[0] = lo.layout; out[1] = lo.tiles_x; out[2] = lo.tiles_y; out[3] = lo.order; out[4] = lo.filter;
}
int stm_set_output(int format, int matrix, int pitch, int uv_row)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (!stm::output_params_ok("set_output", format, matrix, pitch, uv_row)) return -1; // the thread's format stays as it was
    stm::set_output(format == 0 ? stm::Output{0, 0, 0, 0} : stm::Output{format, matrix, pitch, uv_row});
    return 0;
}
void stm_get_output(int out[4])
{
    const stm::Output o = stm::output();
    out[0] = o.format; out[1] = o.matrix; out[2] = o.pitch; out[3] = o.uv_row;
}
int stm_set_overlay(int mode, const unsigned char *d_overlay, int ov_rows, int ov_cols, int x0, int y0, float disparity)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (mode != 0 && mode != 1) // the thread's setting stays as it was
        return STM_REJECT("mode", "set_overlay: mode = %d, must be 0 (off) or 1 (on)", mode) ? 0 : -1;
    if (mode == 1 && !stm::overlay_params_ok("set_overlay", d_overlay, true, ov_rows, ov_cols, x0, y0, disparity)) return -1;
    stm::set_overlay(mode == 0 ? stm::Overlay{0, nullptr, 0, 0, 0, 0, 0.0f} : stm::Overlay{1, d_overlay, ov_rows, ov_cols, x0, y0, disparity});
    return 0;
}
void stm_get_overlay(int out[5], float *disparity)
{
    const stm::Overlay o = stm::overlay();
    out[0] = o.mode; out[1] = o.ov_rows; out[2] = o.ov_cols; out[3] = o.x0; out[4] = o.y0;
    if (disparity) *disparity = o.disparity;
}
int stm_set_overlay_auto(int mode, int near_permille, float margin, int pad, float limit_lo, float limit_hi, float rate_near, float rate_far,
                         float *d_state)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (mode != 0 && mode != 1) // the thread's setting stays as it was
        return STM_REJECT("mode", "set_overlay_auto: mode = %d, must be 0 (off) or 1 (on)", mode) ? 0 : -1;
    if (mode == 1 && !stm::overlay_auto_params_ok("set_overlay_auto", near_permille, margin, pad, limit_lo, limit_hi, rate_near, rate_far)) return -1;
    stm::set_overlay_auto(mode == 0 ? stm::overlay_auto_default()
                                    : stm::OverlayAuto{1, near_permille, margin, pad, limit_lo, limit_hi, rate_near, rate_far, d_state});
    return 0;
}
void stm_get_overlay_auto(int out_mode[3], float out[5])
{
    const stm::OverlayAuto a = stm::overlay_auto();
    out_mode[0] = a.mode; out_mode[1] = a.near_permille; out_mode[2] = a.pad;
    out[0] = a.margin; out[1] = a.limit_lo; out[2] = a.limit_hi; out[3] = a.rate_near; out[4] = a.rate_far;
}
void stm_set_quilt_lds_limit(int bytes) { stm::g_quilt_lds_limit = bytes <= 0 ? 32 * 1024 : (bytes > 64 * 1024 ? 64 * 1024 : bytes); }
int stm_set_packing(int packing, int swap, int filter, int gap)
{
    if (stm::api_outermost()) stm::clear_failed();
    const stm::Packing pk = {packing, swap, filter, gap};
    if (!stm::packing_params_ok("set_packing", pk)) return -1; // the thread's packing stays as it was
    stm::set_packing(pk);
    return 0;
}
void stm_get_packing(int *out)
{
    const stm::Packing pk = stm::packing();
    out[0] = pk.packing; out[1] = pk.swap; out[2] = pk.filter; out[3] = pk.gap;
}
int stm_set_depth(int mode, float gain, float conv)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (!stm::depth_params_ok("set_depth", mode, gain, conv)) return -1; // the thread's setting stays as it was
    stm::Depth d = stm::depth(); // mode 2's parameters (stm_set_depth_auto) are kept
    if (mode == 2 && !(d.disp_lo < d.disp_hi))
        return STM_REJECT("mode", "set_depth: mode 2 (automatic) needs the budget of stm_set_depth_auto first") ? 0 : -1;
    d.mode = mode;
    d.gain = mode == 1 ? gain : 1.0f;
    d.conv = mode == 1 ? conv : 0.0f;
    stm::set_depth(d);
    return 0;
}
int stm_set_depth_auto(float disp_lo, float disp_hi, float max_gain, int clip_permille, float rate, float *d_state)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (!stm::depth_auto_params_ok("set_depth_auto", disp_lo, disp_hi, max_gain, clip_permille, rate)) return -1;
    stm::Depth d = stm::depth();
    d.disp_lo = disp_lo; d.disp_hi = disp_hi; d.max_gain = max_gain; d.clip_permille = clip_permille; d.rate = rate; d.d_state = d_state;
    stm::set_depth(d);
    return 0;
}
int stm_set_antialias(int mode, float strength, int max_radius, float gate)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (mode != 0 && mode != 1) // the thread's setting stays as it was
        return STM_REJECT("mode", "set_antialias: mode = %d, must be 0 (off) or 1 (on)", mode) ? 0 : -1;
    if (mode == 1 && !stm::antialias_params_ok("set_antialias", strength, max_radius, gate)) return -1;
    stm::set_antialias(mode == 0 ? stm::Antialias{0, 0.0f, 0, 0.0f} : stm::Antialias{1, strength, max_radius, gate});
    return 0;
}
void stm_get_antialias(int out_mode[2], float out[2])
{
    const stm::Antialias a = stm::antialias();
    out_mode[0] = a.mode; out_mode[1] = a.max_radius;
    out[0] = a.strength; out[1] = a.gate;
}
int stm_set_align(int mode, float a, float b, float c)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (!stm::align_params_ok("set_align", mode, a, b, c)) return -1; // the thread's setting stays as it was
    stm::Align al = stm::align(); // mode 2's parameters (stm_set_align_auto) are kept
    al.mode = mode;
    al.a = mode == 1 ? a : 0.0f;
    al.b = mode == 1 ? b : 0.0f;
    al.c = mode == 1 ? c : 0.0f;
    stm::set_align(al);
    return 0;
}
int stm_set_align_auto(int radius, float rate, float *d_state)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (!stm::align_auto_params_ok("set_align_auto", radius, rate)) return -1;
    stm::Align al = stm::align();
    al.radius = radius; al.rate = rate; al.d_state = d_state;
    stm::set_align(al);
    return 0;
}
void stm_get_align(int out_mode[2], float out[4])
{
    const stm::Align al = stm::align();
    out_mode[0] = al.mode; out_mode[1] = al.radius;
    out[0] = al.a; out[1] = al.b; out[2] = al.c; out[3] = al.rate;
}
int stm_set_balance(int mode, const unsigned char *lut768)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (!stm::balance_params_ok("set_balance", mode, lut768)) return -1; // the thread's setting stays as it was
    stm::Balance b = stm::balance(); // mode 2's parameters (stm_set_balance_auto) are kept
    b.mode = mode;
    for (int i = 0; i < 768; ++i) b.lut[i] = mode == 1 ? lut768[i] : (unsigned char)i;
    stm::set_balance(b);
    return 0;
}
int stm_set_balance_auto(int max_shift, float rate, int *d_state)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (!stm::balance_auto_params_ok("set_balance_auto", max_shift, rate)) return -1;
    stm::Balance b = stm::balance();
    b.max_shift = max_shift; b.rate = rate; b.d_state = d_state;
    stm::set_balance(b);
    return 0;
}
void stm_get_balance(int out_mode[2], float *out_rate, unsigned char out_lut[768])
{
    const stm::Balance b = stm::balance();
    out_mode[0] = b.mode; out_mode[1] = b.max_shift;
    *out_rate = b.rate;
    memcpy(out_lut, b.lut, 768);
}
int stm_set_cut(int mode, int thresh_permille, int min_gap, int *d_state)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (mode != 0 && mode != 1) // the thread's setting stays as it was
        return STM_REJECT("mode", "set_cut: mode = %d, must be 0 (off) or 1 (on)", mode) ? 0 : -1;
    stm::Cut c = stm::cut(); // mode 0: the other arguments are ignored, the numbers stay
    c.mode = mode;
    if (mode == 1) {
        if (!stm::cut_params_ok("set_cut", thresh_permille, min_gap)) return -1;
        if (!d_state) // without history there is nothing to detect
            return STM_REJECT("d_state", "set_cut: d_state must not be null in mode 1") ? 0 : -1;
        c.thresh_permille = thresh_permille; c.min_gap = min_gap; c.d_state = d_state;
    } else {
        c.d_state = nullptr;
    }
    stm::set_cut(c);
    return 0;
}
void stm_get_cut(int out[3])
{
    const stm::Cut c = stm::cut();
    out[0] = c.mode; out[1] = c.thresh_permille; out[2] = c.min_gap;
}
int stm_set_active(int mode, const int rect[4], int fill, float fill_disp)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (!stm::active_params_ok("set_active", mode, rect, fill, fill_disp)) return -1; // the thread's setting stays as it was
    stm::Active a = stm::active(); // mode 2's parameters (stm_set_active_auto) are kept
    a.mode = mode;
    for (int i = 0; i < 4; ++i) a.rect[i] = mode == 1 ? rect[i] : 0;
    a.fill = mode ? fill : 0;
    a.fill_disp = mode ? fill_disp : 0.0f;
    stm::set_active(a);
    return 0;
}
int stm_set_active_auto(int thresh_luma, int lit_permille, int max_bar_permille, int hold, int *d_state)
{
    if (stm::api_outermost()) stm::clear_failed();
    if (!stm::active_auto_params_ok("set_active_auto", thresh_luma, lit_permille, max_bar_permille, hold)) return -1;
    stm::Active a = stm::active();
    a.thresh_luma = thresh_luma; a.lit_permille = lit_permille; a.max_bar_permille = max_bar_permille; a.hold = hold; a.d_state = d_state;
    stm::set_active(a);
    return 0;
}
void stm_get_active(int out[10], float *fill_disp)
{
    const stm::Active a = stm::active();
    out[0] = a.mode;
    for (int i = 0; i < 4; ++i) out[1 + i] = a.rect[i];
    out[5] = a.fill; out[6] = a.thresh_luma; out[7] = a.lit_permille; out[8] = a.max_bar_permille; out[9] = a.hold;
    *fill_disp = a.fill_disp;
}
int stm_set_agg_tap(float *d_h1, float *d_v2, float *d_h4, const float *d_inject_v2)
{
    if (stm::api_outermost()) stm::clear_failed();
    const void *p[4] = {d_h1, d_v2, d_h4, d_inject_v2};
    const char *name[4] = {"d_h1", "d_v2", "d_h4", "d_inject_v2"};
    for (int i = 0; i < 4; ++i)
        if (((uintptr_t)p[i] & 3) != 0) // the thread's tap stays as it was
            return STM_REJECT(name[i], "set_agg_tap: %s must be 4-byte aligned (a volume of floats)", name[i]) ? 0 : -1;
    stm::set_agg_tap(stm::AggTap{d_h1, d_v2, d_h4, d_inject_v2});
    return 0;
}
void stm_set_agg_variant(int v)
{
#ifndef STM_TIMING
    v -= ((v / 100000) % 10) * 100000; // the timing-experiment digit exists in libstm_hip_timing.so only
#endif
    stm::g_agg_variant = v;
}
}
