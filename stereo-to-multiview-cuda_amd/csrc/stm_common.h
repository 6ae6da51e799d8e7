// stm_common.h -- internal runtime shared by the kernel files and the C-ABI layer.
// gfx950 only.  Not installed; the public surface is include/stm_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <initializer_list>

typedef unsigned char u8;

namespace stm {

// ---- error handling: reference semantics (cuda_utils.h:12-21) = message + exit(1) ----
void fail(const char *what, const char *expr, const char *file, int line);
// A refused argument: fail() with the printf-formatted message and `arg` as its expression.  Returns false, so a screen reads
// `if (bad) return STM_REJECT("arg", "%s: arg = %d, must be ...", fn, arg);` and an entry that answers -1
// `if (bad) return STM_REJECT(...) ? 0 : -1;`.  The macro hands on the rule's own file and line.
bool reject(const char *file, int line, const char *arg, const char *fmt, ...) __attribute__((format(printf, 4, 5)));
#define STM_REJECT(arg, ...) ::stm::reject(__FILE__, __LINE__, arg, __VA_ARGS__)
// the null-pointer rule of a screen: "a must not be null", "a and b must not be null", "a, b and c must not be null" (the names of all
// the pointers, whichever is null; the expression is "a, b, c"); false with the error recorded
struct NamedPtr { const char *name; const void *p; };
bool ptrs_ok(const char *fn, std::initializer_list<NamedPtr> ptrs);
// Error mode 1 (record and return, stm_set_error_mode): a failure is STICKY for the rest of the API call on this thread --
// every later kernel launch of the call is skipped (STM_LAUNCH) and the workspace hands out no memory, so a failed
// allocation can never turn into a kernel running on a null or stale pointer.  Each API entry point clears the flag.
bool failed();
void clear_failed();
struct ApiNest { ApiNest(); ~ApiNest(); }; // held by an entry point around the entry points it calls
bool api_outermost();
void release_host_frame_bufs(); // stm_api.hip: the calling thread's staging buffers of the host-flavour frame calls
// stm_api.hip: the geometry rules of an NV12 frame (include/stm_hip.h); false with the error recorded.  cols_name: the caller's name
// for the width of a view
bool nv12_args_ok(const char *fn, int num_rows, int num_cols_sbs, int num_cols, const char *cols_name, int pitch_y, int pitch_uv, int matrix);
#define STM_CHECK(expr)                                                                  \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) ::stm::fail(hipGetErrorString(_e), #expr, __FILE__, __LINE__); \
    } while (0)
// the reference never checks launches; we do
#define STM_CHECK_LAUNCH() STM_CHECK(hipGetLastError())
#define STM_LAUNCH(...)                                     \
    do {                                                    \
        if (!::stm::failed()) hipLaunchKernelGGL(__VA_ARGS__); \
    } while (0)

hipStream_t stream();
// One word per device, allocated on first use and never freed (so a captured graph can keep its address), zero unless a kernel
// clamped something that cannot happen (see IrvArgs::diag).  stm_last_error() reads and clears it.
uint32_t *device_diag();

// ---- grow-only device workspace, bump-allocated per top-level call -----------------
// The reference hipMalloc/hipFree's ~35 buffers per frame (d_io.cu:43-235); here one
// cached slab is carved up, so a steady-state frame performs no allocation at all.
struct Workspace {
    static void begin(size_t bytes_hint = 0); // start a carve scope (resets the bump pointer)
    static void *alloc(size_t bytes);         // 256-B aligned; grows (sync + realloc) if needed
    template <class T> static T *get(size_t n) { return (T *)alloc(n * sizeof(T)); }
};

void *ws_private_create();
void ws_private_bind(void *ws); // nullptr: back to the thread's shared workspace
void ws_private_destroy(void *ws);
void ws_identity(void **base, size_t *cap);
bool prof_enabled();

// ---- profiling of named kernels with HIP events on the launch stream ----------------
struct ProfScope {
    ProfScope(const char *name);
    ~ProfScope();
    int slot;
    void *ev_b; // end event (kept here: the record vector may be resized by another thread)
};

int agg_variant();
// The display geometry of the lenticular interlacer (stm_set_lens, include/stm_hip.h): mode 0 = off (the reference's interlacer),
// 1 = nearest view, 2 = two views blended, 3 = every sub-pixel rendered at its own continuous position (frame calls only).
// One per host thread; a frame stream installs its own copy around its frame calls (stm_stream_set_lens).
struct Lens {
    int mode;
    double pitch, slope, centre;
};
Lens lens();
void set_lens(const Lens &l);
// the argument rules of a lens geometry with mode in [mode_lo, mode_hi]; false with the error recorded
bool lens_params_ok(const char *fn, int mode, int mode_lo, int mode_hi, double pitch, double slope, double centre);
// The depth budget of the renderer (stm_set_depth / stm_set_depth_auto, include/stm_hip.h): mode 0 = off (the views span the camera
// baseline), 1 = manual (gain, conv), 2 = automatic (gain and conv fitted to the frame's disparity range on the device).  One per
// host thread, next to the lens geometry; a frame stream installs its own copy around its frame calls.
struct Depth {
    int mode;
    float gain, conv;                                // mode 1
    float disp_lo, disp_hi, max_gain, rate;          // mode 2: the budget in view pixels, the gain's ceiling, the state's update rate
    int clip_permille;
    float *d_state;                                  // mode 2: {valid, gain, conv, 0} in device memory; null = scratch, every frame on its own
};
Depth depth();
void set_depth(const Depth &d);
// the argument rules of the two settings; false with the error recorded
bool depth_params_ok(const char *fn, int mode, float gain, float conv);
bool depth_auto_params_ok(const char *fn, float disp_lo, float disp_hi, float max_gain, int clip_permille, float rate);
// The packing of the input frame (stm_set_packing, include/stm_hip.h): where the two eyes lie in the frame and how a squeezed eye is
// expanded.  packing 0 / 1 = side by side full / half width, 2 / 3 = top and bottom full / half height; swap: the right eye comes
// first; filter 0 = linear, 1 = Catmull-Rom (packings 1 and 3); gap: pixels between the eyes along the packing axis.  All 0 = off:
// the reference's layout and the existing kernels.  One per host thread, next to the lens geometry; a frame stream installs its own.
struct Packing {
    int packing, swap, filter, gap;
    bool on() const { return (packing | swap | filter | gap) != 0; }
    int rows_f(int H) const { return packing == 2 ? 2 * H + gap : packing == 3 ? 2 * (H / 2) + gap : H; } // the frame's rows
};
Packing packing();
void set_packing(const Packing &p);
// the rules of the four settings alone (ranges; a filter with a full packing); false with the error recorded
bool packing_params_ok(const char *fn, const Packing &pk);
// stm_api.hip: the four settings and the geometry rules of a packed frame whose unpacked eyes are num_rows x num_cols (stm_hip.h);
// nv12: the evenness rules, the two pitches and the matrix as well.  false with the error recorded.  cols_name: as nv12_args_ok
bool packing_args_ok(const char *fn, const Packing &pk, int num_rows, int num_cols_sbs, int num_cols, const char *cols_name, bool nv12,
                     int pitch_y, int pitch_uv, int matrix);
// a screened packed frame as the kernels of stm_kernels_pack.hip take it: BGR (frame, num_cols_sbs pixels a row) or NV12 planes
struct PackInput {
    Packing pk;
    bool nv12;
    const u8 *frame;
    int num_cols_sbs;
    const u8 *y, *uv;
    int pitch_y, pitch_uv, matrix;
};
// The geometry of the output frame (stm_set_layout, include/stm_hip.h): layout 0 = the interlaced frame (the lens geometry applies),
// 1 = a quilt of tiles_x x tiles_y tiles, one view each; order bit 0: tile rows run bottom-up, bit 1: the view order is reversed;
// filter 0 = the reference's four-neighbour sampler, 1 = the area average.  One per host thread, next to the lens geometry; a frame
// stream installs its own copy around its frame calls (stm_stream_set_layout).
struct Layout {
    int layout, tiles_x, tiles_y, order, filter;
};
Layout layout();
void set_layout(const Layout &l);
// the rules of the five settings alone; false with the error recorded
bool layout_params_ok(const char *fn, int layout, int tiles_x, int tiles_y, int order, int filter);
// stm_api.hip: a quilt's tiling against the views and the output frame (stm_hip.h); false with the error recorded.  views_name,
// rows_name, cols_name: the caller's names for the number of views and the output's size
bool quilt_args_ok(const char *fn, const Layout &lo, int num_views, int in_rows, int in_cols, int out_rows, int out_cols, const char *views_name,
                   const char *rows_name, const char *cols_name);
// The format of the output frame (stm_set_output, include/stm_hip.h): format 0 = BGR (the default), 1 = one NV12 surface -- the Y plane
// of `pitch` bytes a row (0: num_cols_out) from byte 0, the UV plane from row `uv_row` (0: num_rows_out) -- converted by `matrix`.
// One per host thread, next to the layout; a frame stream installs its own copy around its frame calls (stm_stream_set_output).
struct Output {
    int format, matrix, pitch, uv_row;
};
Output output();
void set_output(const Output &o);
// the rules of the four settings alone; false with the error recorded
bool output_params_ok(const char *fn, int format, int matrix, int pitch, int uv_row);
// the integer coefficients of stm_mux_nv12 (stm_hip.h) for `matrix`, and a screened NV12 destination as the kernels take it
struct Nv12OutCoef {
    int yo, yr, yg, yb, h, ur, ug, vg, vb;
};
Nv12OutCoef nv12_out_coef(int matrix);
struct Nv12Out {
    u8 *y, *uv;
    size_t pitch_y, pitch_uv;
    Nv12OutCoef k;
    int pairs; // both planes' bases and pitches are even: a block's two samples of a row leave as one 16-bit store
};
Nv12Out nv12_out(u8 *y, size_t pitch_y, u8 *uv, size_t pitch_uv, int matrix);
// the thread's NV12 surface at `surface` for a frame of Hout x Wout (format 1, screened by the frame call)
Nv12Out nv12_out_surface(u8 *surface, const Output &o, int Hout, int Wout);
// bytes of the thread's output frame: Hout * Wout * elem_sz, or the NV12 surface's pitch * (uv_row + Hout / 2)
size_t frame_out_bytes(int Hout, int Wout, int elem_sz);
// stm_k_mux_nv12 (stm_kernels_dibr.hip): the BGR image img (H x W x elem_sz, H and W even) into o
void launch_mux_nv12(const Nv12Out &o, const u8 *img, int H, int W, int elem_sz);
int quilt_lds_limit(); // stm_set_quilt_lds_limit: the bytes of LDS the area filter's staged kernel may take per workgroup
int irv_paper_ratio(); // stm_set_irv_paper_ratio: accept on count / S instead of the reference's bin index / S (SURVEY A-Q17 iv)
int irv_chunk();       // stm_set_irv_chunk: list entries per wave and trip of stm_k_irv_vote_cm, 0 = the kernel's own rule
// Timing experiments (skip loads / sweeps / stores; results NOT valid) exist only in the separate libstm_hip_timing.so
// (make timing, -DSTM_TIMING): in the product library every STM_DBG test is the constant false and stm_set_agg_variant
// accepts result-preserving variants only.
#ifdef STM_TIMING
#define STM_DBG(dbg, bit) (((dbg) & (bit)) != 0)
static inline int timing_knobs() { return (agg_variant() / 100000) % 10; }
#else
#define STM_DBG(dbg, bit) false
static inline int timing_knobs() { return 0; }
#endif

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// A cost volume as the kernels see it: either the reference's table of plane pointers
// (T1 in SURVEY 8a; `tab` is a DEVICE array of D device pointers) or a dense slab
// [D][H][W] (`base` + d * plane_stride).  One branch per plane access, uniform per wave.
// Third form, internal to the frame pipeline: QUADS = float4 [ceil(D/4)][H][W], the four hypotheses
// 4q..4q+3 of a pixel interleaved in one 16-byte element (`plane_stride` counts float4 elements).
struct Vol {
    float *const *tab;
    float *base;
    size_t plane_stride;
    int quad;
    __device__ __forceinline__ float *plane(int d) const { return tab ? tab[d] : base + (size_t)d * plane_stride; }
};
static inline Vol vol_table(float **d_tab) { Vol v; v.tab = d_tab; v.base = nullptr; v.plane_stride = 0; v.quad = 0; return v; }
static inline Vol vol_slab(float *base, size_t stride) { Vol v; v.tab = nullptr; v.base = base; v.plane_stride = stride; v.quad = 0; return v; }
static inline Vol vol_quads(float *base, size_t stride) { Vol v; v.tab = nullptr; v.base = base; v.plane_stride = stride; v.quad = 1; return v; }

#ifdef __HIPCC__
// Target column of a caller's map value: clamp(x + sd, 0, W - 1) (map_col) or clamp(x - sd, 0, W - 1) (map_col_sub), the sum
// taken without overflow.  sd is a float -> int conversion (v_cvt_i32_f32: truncates, saturates at INT_MIN / INT_MAX, NaN -> 0),
// so x + INT_MAX and x - INT_MIN would wrap in a 32-bit register; a shift bounded to [-W, W] first lands on the same column
// (x is in [0, W): anything at or beyond +-W leaves the row on that side).  Same column as before for every |sd| < 2^31 - W.
__device__ __forceinline__ int map_col(int x, int sd, int W) { return min(max(x + min(max(sd, -W), W), 0), W - 1); }
__device__ __forceinline__ int map_col_sub(int x, int sd, int W) { return min(max(x - min(max(sd, -W), W), 0), W - 1); }

// A "quad" = the four hypotheses d0..d0+3 of one pixel.  PLANES layout: four dword accesses, one per
// plane (each wave instruction is a contiguous 256-B row segment).  QUADS layout (internal to the frame
// pipeline, Vol::quad): one 16-byte access.
template <bool QUAD> __device__ __forceinline__ float4 load_quad(const Vol &v, int q, int D, size_t idx)
{
    if (QUAD) { // the volume is streamed: each element is read once per pass, so do not let it displace the arm planes in L2
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f t = __builtin_nontemporal_load((const v4f *)v.base + (size_t)q * v.plane_stride + idx);
        return make_float4(t.x, t.y, t.z, t.w);
    }
    const int d0 = q * 4;
    float4 r;
    r.x = v.plane(d0)[idx];
    r.y = d0 + 1 < D ? v.plane(d0 + 1)[idx] : 0.f;
    r.z = d0 + 2 < D ? v.plane(d0 + 2)[idx] : 0.f;
    r.w = d0 + 3 < D ? v.plane(d0 + 3)[idx] : 0.f;
    return r;
}
// STREAM: non-temporal store (the aggregation passes: measured 3-5 % faster; the cost-init kernel, which only writes, is
// 10 % slower with it and keeps ordinary stores)
template <bool QUAD, bool STREAM = true> __device__ __forceinline__ void store_quad(const Vol &v, int q, int D, size_t idx, float4 s)
{
    if (QUAD && !STREAM) { ((float4 *)v.base)[(size_t)q * v.plane_stride + idx] = s; return; }
    if (QUAD) { // written once, read by the next pass from HBM (530 MB >> L2): streaming store
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f t = {s.x, s.y, s.z, s.w};
        __builtin_nontemporal_store(t, (v4f *)v.base + (size_t)q * v.plane_stride + idx);
        return;
    }
    const int d0 = q * 4;
    v.plane(d0)[idx] = s.x;
    if (d0 + 1 < D) v.plane(d0 + 1)[idx] = s.y;
    if (d0 + 2 < D) v.plane(d0 + 2)[idx] = s.z;
    if (d0 + 3 < D) v.plane(d0 + 3)[idx] = s.w;
}

#endif

// ---- launchers (one per kernel family; definitions next to the kernels) -------------
// cost init (stm_kernels_cost.hip)
void launch_pack_bgrx(const u8 *bgr, uint32_t *packed, int H, int W, int elem_sz);
void launch_census32_pair(const uint32_t *packed_l, uint32_t *census_l, const uint32_t *packed_r, uint32_t *census_r, int H, int W);
// frame pipeline: launch_demux_sbs_packed + launch_census32_pair in one kernel (Wsbs >= 2 W)
void launch_front(u8 *l, u8 *r, uint32_t *pk_l, uint32_t *pk_r, uint32_t *wide_l, uint32_t *wide_r, uint32_t *cen_l, uint32_t *cen_r,
                  const u8 *sbs, int H, int Wsbs, int W, int elem_sz);
// NV12 input (y: H rows of pitch_y bytes, uv: H / 2 rows of pitch_uv bytes; H, W even, pitches >= 2 W, matrix 0 .. 3, all
// screened by the caller): launch_front on the converted frame, and the plain converter + split
void launch_front_nv12(u8 *l, u8 *r, uint32_t *pk_l, uint32_t *pk_r, uint32_t *wide_l, uint32_t *wide_r, uint32_t *cen_l, uint32_t *cen_r,
                       const u8 *y, int pitch_y, const u8 *uv, int pitch_uv, int H, int W, int elem_sz, int matrix);
void launch_demux_nv12(u8 *l, u8 *r, const u8 *y, int pitch_y, const u8 *uv, int pitch_uv, int H, int W, int elem_sz, int matrix);
// the reduced-resolution frame's front in one launch: the full-size split images l / r (H x W), the bilinearly reduced images
// low_l / low_r (h x w, bit for bit launch_scale_bilinear of the split images) and the reduced pair's BGRX, wide and census planes
// (launch_front's formats).  sbs != nullptr: a side-by-side BGR frame, Wsbs >= 2 W; otherwise the NV12 planes of launch_front_nv12
void launch_front_low(u8 *l, u8 *r, u8 *low_l, u8 *low_r, uint32_t *pk_l, uint32_t *pk_r, uint32_t *wide_l, uint32_t *wide_r, uint32_t *cen_l,
                      uint32_t *cen_r, const u8 *sbs, int Wsbs, const u8 *y, int pitch_y, const u8 *uv, int pitch_uv, int matrix, int H, int W,
                      int h, int w, int elem_sz);
// packed input (stm_kernels_pack.hip; `in` screened by packing_args_ok): the two unpacked eyes H x W x elem_sz as a stage, and
// launch_front on the unpacked frame without materialising it
void launch_demux_packed(u8 *l, u8 *r, const PackInput &in, int H, int W, int elem_sz);
void launch_front_pack(u8 *l, u8 *r, uint32_t *pk_l, uint32_t *pk_r, uint32_t *wide_l, uint32_t *wide_r, uint32_t *cen_l, uint32_t *cen_r,
                       const PackInput &in, int H, int W, int elem_sz);
void launch_cost_init(const uint32_t *pk_l, const uint32_t *pk_r, const uint32_t *cen_l, const uint32_t *cen_r,
                      Vol cost_l, Vol cost_r, const float *lut_ad, const float *lut_census,
                      int D, int zd, int H, int W);
void launch_cost_quirks(const uint32_t *pk_l, const uint32_t *pk_r, const uint32_t *cen_l, const uint32_t *cen_r, Vol cost_l,
                        Vol cost_r, const float *lut_ad, const float *lut_census, int D, int zd, int H, int W);
int ref_quirks(); // stm_set_ref_quirks
// aggregation (stm_kernels_agg.hip)
void launch_cross_arms(const uint32_t *packed, u8 *up, u8 *down, u8 *left, u8 *right,
                       float ucd, float lcd, int usd, int lsd, int H, int W);
void launch_cross_arms2(int nviews, const uint32_t *const *packed, u8 *const *up, u8 *const *down, u8 *const *left,
                        u8 *const *right, float ucd, float lcd, int usd, int lsd, int H, int W, const uint32_t *const *wide_ready = nullptr,
                        uint32_t *htab = nullptr, // htab: also build stm_k_pq_hsr's horizontal window table (aggh_table_dwords(nviews, H, W))
                        uint32_t *vtab = nullptr, int vrec = 0, int vtop = -1, // + vtab: and the vertical one of the register-ring kernel (aggm_frame_vtab_dwords)
                        bool vcol = false);                                    // vcol: in stm_k_pq_v12r's per-column layout (stm_hwin.h)
void launch_agg_h(Vol in, Vol out, const u8 *armL, const u8 *armR, int D, int H, int W);
void launch_agg_v(Vol in, Vol out, const u8 *armU, const u8 *armD, int D, int H, int W, int usd);
void launch_agg_h2(Vol in_a, Vol out_a, const u8 *armL_a, const u8 *armR_a, Vol in_b, Vol out_b, const u8 *armL_b, const u8 *armR_b,
                   int D, int H, int W);
void launch_agg_h2_cost(const uint32_t *pk_l, const uint32_t *cen_l, const uint32_t *pk_r, const uint32_t *cen_r, const float *lut,
                        Vol out_l, const u8 *armL_l, const u8 *armR_l, Vol out_r, const u8 *armL_r, const u8 *armR_r, int D, int zd,
                        int H, int W);
void launch_agg_h_wta2(Vol in_a, const u8 *armL_a, const u8 *armR_a, float *disp_a, Vol in_b, const u8 *armL_b, const u8 *armR_b,
                       float *disp_b, int D, int zd, int H, int W);
void launch_wta(Vol cost, float *disp, int D, int zd, int H, int W);
// refinement (stm_kernels_refine.hip)
void launch_dcc(u8 *out_l, u8 *out_r, const float *disp_l, const float *disp_r, u8 *hit_l, u8 *hit_r, int H, int W);
// nviews = 1 or 2 (both views of a frame share every launch); scratch comes from the current Workspace scope
// (16 bytes per pixel per view).  with_dcc (frame pipeline, nviews = 2): the L/R check of disp[0] / disp[1] runs first and fills
// outl[0] / outl[1] -- fused with the first region-voting pass where that form applies, as launch_dcc_rows otherwise
void launch_irv(int nviews, float *const *disp, u8 *const *outl, const u8 *const *up, const u8 *const *down,
                const u8 *const *left, const u8 *const *right, int thresh_s, float thresh_h,
                int H, int W, int D, int zd, int usd, int iterations, bool device_flavour, bool with_dcc = false);
// what launch_irv runs for these arguments, as stm_irv_path's bit field (include/stm_hip.h); launches nothing
int irv_path(int H, int W, int usd, int iterations, bool device_flavour, bool with_dcc);
void launch_bilateral(const float *in, float *out, const float *spatial, const float *color,
                      int radius, int H, int W, int D);
// integer_maps: both maps hold integer-valued disparities any two of which differ by less than D (the frame pipeline's own
// WTA / region-voting output)
void launch_bilateral2(const float *in_a, float *out_a, const float *in_b, float *out_b, const float *spatial, const float *color,
                       int radius, int H, int W, int D, bool integer_maps = false, const float *one_value = nullptr, int zd = 0);
void launch_gaussian_max(const float *in, float *out, const float *spatial, int radius, float sigma, int H, int W,
                         bool invert_input);
// sub-pixel enhancement (stm_kernels_subpix.hip): disp refined in place from the materialised volume (per-stage call), or in
// the frame pipeline from the last horizontal pass's input -- PQ volumes (pq) or quads (quads, when pq == nullptr) -- of both views
void launch_subpix(Vol cost, float *disp, int D, int zd, int H, int W);
void launch_subpix_frame(float *const *pq, float *const *quads, float *const *disp, const u8 *const *armL, const u8 *const *armR, int D,
                         int zd, int H, int W);
// outlier interpolation (stm_kernels_interp.hip): disp[v] refined in place where outl[v] != 0, from the reliable pixels (outl[v] == 0)
// along 16 directions and the view's own image; nviews = 1 or 2 in one launch
void launch_interp(int nviews, float *const *disp, const u8 *const *outl, const u8 *const *img, int H, int W, int elem_sz);
// DIBR + mux (stm_kernels_dibr.hip)
void launch_demux_sbs(u8 *l, u8 *r, const u8 *sbs, int H, int Wsbs, int W, int elem_sz);
// same, and the BGRX dwords (launch_pack_bgrx) + wide pixels (launch_cross_arms2) of both halves in the same pass
void launch_demux_sbs_packed(u8 *l, u8 *r, uint32_t *pk_l, uint32_t *pk_r, uint32_t *wide_l, uint32_t *wide_r, const u8 *sbs, int H,
                             int Wsbs, int W, int elem_sz);
void launch_occl(u8 *occl_l, u8 *occl_r, const float *disp_l, const float *disp_r, int H, int W);
void launch_bleed(const u8 *in, u8 *out, int radius, int H, int W);
void launch_median3(const float *in, float *out, int H, int W);
void launch_dcc_rows(u8 *out_l, u8 *out_r, const float *disp_l, const float *disp_r, int H, int W);
void launch_hitmask_rows(float *mask_l, float *mask_r, const float *disp_l, const float *disp_r, int H, int W);
void launch_occl_to_mask(float *mask_l, float *mask_r, const u8 *occl_l, const u8 *occl_r, int H, int W);
void launch_view_synth(u8 *out, const u8 *img_l, const u8 *img_r, const float *disp_l, const float *disp_r,
                       const float *mask_l, const float *mask_r, const float *blend, float shift, int H, int W, int elem_sz,
                       bool linear = false); // linear: warp_tap<true>, the fractional fetch of stm_dibr_dbm_lin / frame bit 0x800
void launch_view_synth_all(u8 *views, size_t view_stride, int N, const u8 *img_l, const u8 *img_r, const float *disp_l,
                           const float *disp_r, const float *mask_l, const float *mask_r, const float *blend, int H, int W,
                           int elem_sz, bool linear = false);
void launch_fwarp(u8 *out, const u8 *img, const float *disp, float shift, unsigned long long *keys, int H, int W, int elem_sz);
void launch_scale_bilinear(const u8 *in, u8 *out, int in_rows, int in_cols, int out_rows, int out_cols, int elem_sz);
void launch_disp_scale(float *out, const float *in, int out_rows, int out_cols, int in_rows, int in_cols, float disp_scale);
void launch_view_table(u8 **tab, u8 *first, u8 *last, u8 *mem, size_t stride, int N);
// guided disparity up-sampling (stm_kernels_upsample.hip): out[v] (H x W) from the low-resolution map dlow[v] and image ilow[v]
// (h x w) and the guide image img[v] (H x W), v < nviews (1 or 2) in one launch; tab = the 766 colour weights of sigma_color
void launch_disp_upsample(int nviews, float *const *out, const float *const *dlow, const u8 *const *ilow, const u8 *const *img,
                          const float *tab, int H, int W, int h, int w, int elem_sz, float up);
// temporal disparity stabilisation (stm_kernels_temporal.hip): cur[v] (H x W) blended in place towards prev[v] where the 3 x 3
// maximum of the colour change between img[v] and img_prev[v] and the change of the disparity stay inside the gates; v < nviews
// (1 or 2) in one launch.  Pixel (x, y) of view v's images lies at base + byte_off[v] + ((size_t)y * stride + x) * elem_sz
void launch_disp_temporal(int nviews, float *const *cur, const float *const *prev, const u8 *const *img, const u8 *const *img_prev,
                          const size_t *byte_off, int H, int W, int stride, int elem_sz, float alpha, int thresh_color, float thresh_disp);
// the maps of a frame stream as depth planes (stm_kernels_dplane.hip; stm_stream_maps' definition): plane dst[v] of HW codes, u8
// (bytes_per_code 1) or little-endian u16 (2), from the float map src[v]; v < nviews (1 or 2) in one launch.  dst[v] may lie at any
// address that is a multiple of bytes_per_code; k = (float)(maxcode / ((double)hi - lo)) is the host's
void launch_disp_plane(int nviews, const float *const *src, void *const *dst, size_t HW, int bytes_per_code, float lo, float k);
// The image-plus-depth input of a frame stream (stm_stream_input_depth, include/stm_depth_input.h): format -1 = off, 0 = f32, 2 = u8,
// 3 = u16 planes between lo and hi; fill and gate of step E
struct DepthInput {
    int format;
    float lo, hi;
    int fill;
    float gate;
};
// the second eye (stm_kernels_eye.hip; steps A to E of the definition): from the image `img` (H rows of pitch_px pixels, the first W
// read) and the tight plane, the decoded map disp_l, the synthesised img_r and disp_r, and the tight copy img_l of the image (null
// where pitch_px == W).  plane, img_r, disp_l and disp_r 16-byte aligned, W <= 8192
void launch_depth_eye(const u8 *img, int pitch_px, const void *plane, int format, float lo, float hi, int fill, float gate, u8 *img_l,
                      u8 *img_r, float *disp_l, float *disp_r, int H, int W, int elem_sz);
// stm_api.hip: the body of a stream's image-plus-depth frame -- the cut and active-area detectors on the given image, the second eye,
// the active fill and the stereo body's own tail; no matcher.  stages 3 or 3 | 0x800.  No extern "C" entry calls it: a frame entry
// would have to join the recorded screening tables.  Errors are recorded like a frame entry's
void depth_frame_device(const u8 *d_img, const void *d_plane, const DepthInput &di, float *d_disp_l, float *d_disp_r, u8 *d_interlaced,
                        int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out, int elem_sz, int num_views,
                        float angle, int stages);
// The packed 2D-plus-depth video input of a frame stream (stm_stream_input_packed_depth, include/stm_depth_video.h): format -1 = off, 0 =
// BGR, 1 = NV12 frame converted by `matrix`; pk: where the image (eye 0) and the depth picture (eye 1) lie; range, dfilter, dgate, lo,
// hi: steps A' to A'''; fill and gate of step E
struct DepthVideo {
    int format, matrix;
    Packing pk;
    int range, dfilter, dgate;
    float lo, hi;
    int fill;
    float gate;
};
// the second eye of such a frame (stm_kernels_eye.hip, stm_k_eye_video): `in` is the screened frame under dv.pk; the tight BGR image
// img_l, the decoded map disp_l, the synthesised img_r and disp_r, all 16-byte aligned; W <= 8192
void launch_depth_eye_video(const PackInput &in, const DepthVideo &dv, u8 *img_l, u8 *img_r, float *disp_l, float *disp_r, int H, int W,
                            int elem_sz);
// stm_api.hip: the body of a stream's packed 2D-plus-depth frame: depth_frame_device with the packed frame in place of the image and
// the plane (NV12: the UV plane at byte rows_f * num_cols_sbs, both pitches num_cols_sbs).  No extern "C" entry calls it either
void depth_video_frame_device(const u8 *d_frame, const DepthVideo &dv, float *d_disp_l, float *d_disp_r, u8 *d_interlaced, int num_rows,
                              int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out, int elem_sz, int num_views, float angle,
                              int stages);
// frame pipeline: the N - 2 views are synthesised inside the interlacer, sample by sample (no view buffers)
void launch_synth_mux(const u8 *img_l, const u8 *img_r, const float *disp_l, const float *disp_r, const float *mask_l, const float *mask_r,
                      const float *blend, u8 *out, int N, float y_interval, float inv_y_interval, int ymod, int Hin, int Win, int Hout,
                      int Wout, int elem_sz, int variant, bool linear = false);
void launch_mux(const u8 *const *d_views, u8 *out, int N, float y_interval, float inv_y_interval, int ymod,
                int Hin, int Win, int Hout, int Wout, int elem_sz, int variant);
// the lenticular interlacer (stm_set_lens): launch_mux on a table of views (ln.mode 1 or 2) and launch_synth_mux (ln.mode 1, 2 or 3)
// with each sub-pixel's view taken from its lens phase
void launch_mux_lens(const u8 *const *d_views, u8 *out, int N, const Lens &ln, int Hin, int Win, int Hout, int Wout, int elem_sz);
void launch_synth_mux_lens(const u8 *img_l, const u8 *img_r, const float *disp_l, const float *disp_r, const float *mask_l,
                           const float *mask_r, const float *blend, u8 *out, int N, const Lens &ln, int Hin, int Win, int Hout, int Wout,
                           int elem_sz, bool linear);
// the depth budget (stm_set_depth): launch_synth_mux / launch_synth_mux_lens with every view's shift and sampling position mapped
// through gain and conv (ln.mode 0: the reference's view assignment from inv_y_interval and ymod); state != nullptr: gain and conv
// are read from state[1] and state[2] on the device
void launch_synth_mux_depth(const u8 *img_l, const u8 *img_r, const float *disp_l, const float *disp_r, const float *mask_l,
                            const float *mask_r, const float *blend, u8 *out, int N, const Lens &ln, float inv_y_interval, int ymod,
                            float gain, float conv, const float *state, int Hin, int Win, int Hout, int Wout, int elem_sz, bool linear);
// the quilt (stm_set_layout, lo.layout == 1, screened by quilt_args_ok): a table of finished views tiled into `out`, and the frame's
// renderer tiled directly with no view written (depth_mode 0: synth_sample's views; 1, 2: the depth budget's, state as above)
void launch_quilt(const u8 *const *d_views, u8 *out, int N, const Layout &lo, int Hin, int Win, int Hout, int Wout, int elem_sz);
// nv != nullptr (stm_set_output, format 1; every tile and remainder even): the same pixels leave as NV12 into *nv and `out` is not used
void launch_synth_quilt(const u8 *img_l, const u8 *img_r, const float *disp_l, const float *disp_r, const float *mask_l, const float *mask_r,
                        const float *blend, u8 *out, int N, const Layout &lo, int depth_mode, float gain, float conv, const float *state,
                        int Hin, int Win, int Hout, int Wout, int elem_sz, bool linear, const Nv12Out *nv = nullptr);
// The overlay composited into finished frames (stm_set_overlay, include/stm_hip.h): mode 0 = off, 1 = every rendering frame call
// composites `d_overlay` (ov_rows x ov_cols x 4 bytes B, G, R, A premultiplied, device memory the caller keeps alive) as its last
// launch.  One per host thread; a frame stream composites its own after its frame calls and never installs it here.
struct Overlay {
    int mode;
    const u8 *d_overlay;
    int ov_rows, ov_cols, x0, y0;
    float disparity;
    // the disparity read on the device instead (stm_set_overlay_auto): fminf(fmaxf(*d_disp, limit_lo), limit_hi); null = `disparity`
    const float *d_disp = nullptr;
    float limit_lo = 0.0f, limit_hi = 0.0f;
};
Overlay overlay();
void set_overlay(const Overlay &o);
// the rules of an overlay's own arguments (stm_hip.h, stm_mux_overlay); check_ptr: the pointer's too.  false with the error recorded
bool overlay_params_ok(const char *fn, const void *ov, bool check_ptr, int ov_rows, int ov_cols, int x0, int y0, float disparity);
// stm_api.hip: an overlay composited on a finished frame rendered under ln and lo, which the frame call has screened (the frame
// calls' last launch with the thread's settings, and a frame stream's after its frame call with the stream's own)
void frame_overlay(u8 *d_frame, const Overlay &ov, const Lens &ln, const Layout &lo, int num_views, float angle, int Hout, int Wout,
                   int elem_sz);
// the compositor (stm_kernels_overlay.hip): `ov` in place on the finished frame `out` (Hout x Wout x elem_sz); lo.layout 0: interlaced
// under ln (ln.mode 0: the reference's view assignment from y_interval, inv_y_interval and ymod), 1: a quilt.  Screened by the caller
// d_disp != nullptr: the disparity is *d_disp clamped to [limit_lo, limit_hi] on the device (a NaN goes to limit_lo) and the bounding
// box is sized from the limits; the columns that adds sample (0, 0, 0, 0) and leave the frame as it is
void launch_overlay(u8 *out, const u8 *ov, int ov_rows, int ov_cols, int x0, int y0, float disparity, int N, const Lens &ln,
                    float y_interval, float inv_y_interval, int ymod, const Layout &lo, int Hout, int Wout, int elem_sz,
                    const float *d_disp = nullptr, float limit_lo = 0.0f, float limit_hi = 0.0f);
// The overlay's automatic depth placement (stm_set_overlay_auto, include/stm_hip.h): mode 0 = off (not one launch changes), 1 = every
// rendering frame call with the thread's overlay on fits the overlay's disparity to the maps under it on the device and composites
// with the state's disparity.  One per host thread, next to the overlay; a frame stream keeps its own and never installs it here.
struct OverlayAuto {
    int mode;
    int near_permille;
    float margin;
    int pad;
    float limit_lo, limit_hi, rate_near, rate_far;
    float *d_state; // {valid, disparity, nearest, 0} in device memory; null = scratch, every frame on its own
};
OverlayAuto overlay_auto_default();
OverlayAuto overlay_auto();
void set_overlay_auto(const OverlayAuto &a);
// the argument rules of the seven parameters; false with the error recorded
bool overlay_auto_params_ok(const char *fn, int near_permille, float margin, int pad, float limit_lo, float limit_hi, float rate_near,
                            float rate_far);
// the fit's frame rule: num_rows * num_cols < 2^31 (n <= 2 H W is counted in 32 bits); false with the error recorded
bool overlay_fit_size_ok(const char *fn, int num_rows, int num_cols);
constexpr size_t OVERLAY_FIT_WS_WORDS = 4096 + 4; // the histogram, then the alpha box
// the measurement (stm_kernels_ovfit.hip): the alpha box of `ov`, both maps (H x W) under its footprint in the view Hv x Wv into the
// histogram, the fit and the update of `state` (four floats).  The budget is (gain, conv), or depth_state[1], depth_state[2] read on
// the device where depth_state != nullptr; fresh: the state's history is ignored; zero_state: `state` is scratch, zeroed first;
// cut_state: the detector's state or null; d_rect: the active rectangle (four ints in device memory) the footprint is moved into, or null
void launch_overlay_fit(float *state, uint32_t *ws, const float *disp_l, const float *disp_r, int H, int W, const u8 *ov, int ov_rows,
                        int ov_cols, int x0, int y0, int Hv, int Wv, float gain, float conv, const float *depth_state, const OverlayAuto &oa,
                        bool fresh, bool zero_state, const int *cut_state, const int *d_rect = nullptr);
// stm_api.hip: the fit of the overlay `ov` on a frame's maps under layout lo, then the overlay composited at the state's disparity;
// state: oa.d_state, or four floats of scratch (zero_state).  The frame calls' tail with the thread's settings, and a frame stream's with its own
void frame_overlay_auto(u8 *d_frame, const Overlay &ov, const OverlayAuto &oa, float *state, uint32_t *ws, bool fresh, bool zero_state, const float *d_disp_l,
                        const float *d_disp_r, int H, int W, const Depth &dp, const float *depth_state, const int *cut_state, const Lens &ln,
                        const Layout &lo, int num_views, float angle, int Hout, int Wout, int elem_sz, const int *d_rect = nullptr);
// View antialiasing (stm_set_antialias, include/stm_hip.h): mode 0 = off, 1 = every rendering frame call filters both images by
// their own maps (stm_view_prefilter's rule) before it renders from them.  One per host thread, next to the depth budget; a frame
// stream installs its own copy around its frame calls (stm_stream_set_antialias).
struct Antialias {
    int mode;
    float strength;
    int max_radius;
    float gate;
};
Antialias antialias();
void set_antialias(const Antialias &a);
// the rules of the three parameters (stm_hip.h, stm_view_prefilter); false with the error recorded
bool antialias_params_ok(const char *fn, float strength, int max_radius, float gate);
// the prefilter (stm_kernels_prefilter.hip): out[i] = in[i] (H x W x elem_sz) filtered by disp[i], i < nimg (1 or 2) in one launch;
// state != nullptr: gain and conv are read from state[1] and state[2] on the device.  Screened by the caller
void launch_view_prefilter(int nimg, u8 *const *out, const u8 *const *in, const float *const *disp, int H, int W, int elem_sz, int num_views,
                           float strength, int max_radius, float gate, float gain, float conv, const float *state);
// the measurement (stm_kernels_depth.hip): both maps into the 4096-bin histogram `hist` (scratch), the fit, the update of `state`
// (four floats); fresh: the state's history is ignored; d_rect: the active rectangle (four ints in device memory) the count is
// restricted to, or null
void launch_depth_fit(float *state, uint32_t *hist, const float *disp_l, const float *disp_r, int H, int W, float disp_lo, float disp_hi,
                      float max_gain, int clip_permille, float rate, bool fresh, const int *d_rect = nullptr);
// The vertical alignment of the pair (stm_set_align / stm_set_align_auto, include/stm_hip.h): mode 0 = off (not one launch changes),
// 1 = manual (the field a, b, c), 2 = automatic (the field measured on each frame on the device).  One per host thread, next to the
// depth budget; a frame stream installs its own copy around its frame calls.
struct Align {
    int mode;
    float a, b, c;      // mode 1
    int radius;         // mode 2: the search radius in rows, the state's update rate
    float rate;
    float *d_state;     // mode 2: {valid, a, b, c} in device memory; null = scratch, every frame on its own
};
Align align();
void set_align(const Align &a);
// the argument rules of the two settings; false with the error recorded
bool align_params_ok(const char *fn, int mode, float a, float b, float c);
bool align_auto_params_ok(const char *fn, int radius, float rate);
// the measurement's frame rules: num_rows >= 4, num_cols >= 8, and a size whose sums fit 32 bits; false with the error recorded
bool align_size_ok(const char *fn, int num_rows, int num_cols);
// the measurement (stm_kernels_align.hip) of a screened frame (in != nullptr) or of two unpacked images H x W x elem_sz: the profiles
// into prof (align_profile_words(H) words), the SADs into sad (align_sad_words(radius) words), the fit, the update of `state` (four
// floats) and the number of valid blocks into nvalid (may be null); fresh: the state's history is ignored
size_t align_profile_words(int H);
size_t align_sad_words(int radius);
void launch_align_measure(float *state, int *nvalid, uint32_t *prof, uint32_t *sad, const PackInput *in, const u8 *img_l, const u8 *img_r,
                          int H, int W, int elem_sz, int radius, float rate, bool fresh);
// the field applied: a screened frame (in != nullptr) as the aligned side-by-side BGR frame `out` (H x 2 W x elem_sz, the left eye
// copied), or the one image img (H x W x elem_sz) into out; state != nullptr: a, b, c are read from state[1 .. 3] on the device
void launch_align_frame(u8 *out, const PackInput *in, const u8 *img, int H, int W, int elem_sz, float a, float b, float c, const float *state);
// Rectification from camera calibration (stm_stream_rectify, include/stm_rectify.h): mode 0 = off (not one launch changes), 1 = both
// eyes remapped through their records of 18 floats (rec[0] the left eye's, rec[1] the right's) ahead of everything else a frame
// call does.  One per host thread, but no exported setter: a frame stream installs its own copy around its frame calls.
struct Rectify {
    int mode;
    float rec[2][18];
    int border; // 0 = taps outside the eye are 0, 1 = their coordinates are clamped
};
Rectify rectify();
void set_rectify(const Rectify &r);
// the rules of a record and a border; false with the error recorded
bool rectify_params_ok(const char *fn, const float *rec18, int border);
// the remap (stm_kernels_rectify.hip).  A screened frame (in != nullptr): both eyes, unpacked and converted, through rec[0] and rec[1]
// into the side-by-side BGR frame `out` (H x 2 W x elem_sz; 16-byte aligned with 3- or 4-byte pixels: dword or wider stores, a
// 4-byte pixel's last byte written 0).  in == nullptr: the one image img (H x W x elem_sz) through rec[0] into out, at any address; of a pixel of more than
// three bytes the first three are written
void launch_rectify_frame(u8 *out, const PackInput *in, const u8 *img, int H, int W, int elem_sz, const float (*rec)[18], int border);
// the test tap: (qu, qv) per pixel of one eye, INT32_MIN twice where the pixel is not ok
void launch_rectify_coords(int *quv, int H, int W, const float *rec18);
// The colour balance between the eyes (stm_set_balance / stm_set_balance_auto, include/stm_hip.h): mode 0 = off (not one launch
// changes), 1 = given (the right eye through the three tables lut), 2 = measured (the tables fitted on each frame on the device).
// One per host thread, next to the alignment; a frame stream installs its own copy around its frame calls.
struct Balance {
    int mode;
    u8 lut[768];        // mode 1: B, G, R, 256 bytes each (the identity otherwise)
    int max_shift;      // mode 2: the largest shift of a level, the state's update rate
    float rate;
    int *d_state;       // mode 2: {valid, 768 levels in 1/256} in device memory; null = scratch, every frame on its own
};
Balance balance_default();
Balance balance();
void set_balance(const Balance &b);
// the argument rules of the two settings; false with the error recorded
bool balance_params_ok(const char *fn, int mode, const u8 *lut768);
bool balance_auto_params_ok(const char *fn, int max_shift, float rate);
// the measurement's frame rule: num_rows * num_cols < 2^31; false with the error recorded
bool balance_size_ok(const char *fn, int num_rows, int num_cols);
// rate in 1/256: clamp((int)floorf(rate * 256 + 0.5f), 1, 256)
int balance_rate_q(float rate);
constexpr size_t BALANCE_HIST_WORDS = 1536, BALANCE_STATE_WORDS = 769;
// the measurement (stm_kernels_balance.hip) of a screened frame (in != nullptr) or of two unpacked images H x W x elem_sz: the six
// histograms into hist (1536 words), the fit and the update of `state` (769 ints); fresh: the state's history is ignored
void launch_balance_measure(int *state, uint32_t *hist, const PackInput *in, const u8 *img_l, const u8 *img_r, int H, int W, int elem_sz,
                            int max_shift, int rate_q, bool fresh);
// the tables applied: a screened frame (in != nullptr) as the balanced side-by-side BGR frame `out` (H x 2 W x elem_sz, the left eye
// copied), or the one image img (H x W x elem_sz) into out; the tables are lut768 (host memory), or state's (device) where state != nullptr
void launch_balance_frame(u8 *out, const PackInput *in, const u8 *img, int H, int W, int elem_sz, const u8 *lut768, const int *state);
// The shot-change detector (stm_set_cut, include/stm_hip.h): mode 0 = off (not one launch changes), 1 = on: every frame call first
// takes the left eye's signature, decides against the state and, on a cut, zeroes the `valid` word of the recursive states in force.
// One per host thread, next to the balance; a frame stream installs its own copy around its frame calls.
struct Cut {
    int mode;
    int thresh_permille, min_gap;
    int *d_state;       // mode 1: {valid, cut, since, score, sig[256]} in device memory, never null
};
Cut cut_default();
Cut cut();
void set_cut(const Cut &c);
// the argument rules of the detector's two numbers; false with the error recorded
bool cut_params_ok(const char *fn, int thresh_permille, int min_gap);
// the detector's frame rule: num_rows, num_cols >= 4 and num_rows * num_cols < 2^31; false with the error recorded
bool cut_size_ok(const char *fn, int num_rows, int num_cols);
constexpr size_t CUT_SIG_WORDS = 256, CUT_STATE_WORDS = 260;
constexpr int CUT_DEFAULT_THRESH = 370; // the geometric mean of the largest non-cut and the smallest cut score
// the detector (stm_kernels_cut.hip) on the left eye of a screened frame (in != nullptr) or on one unpacked image H x W x elem_sz:
// the signature into sig (256 words), the decision and the update of `state` (260 ints); on a cut one 32-bit zero into each
// non-null reset pointer
void launch_cut_detect(int *state, uint32_t *sig, const PackInput *in, const u8 *img_l, int H, int W, int elem_sz, int thresh_permille,
                       int min_gap, void *reset0, void *reset1, void *reset2);
// The active picture area (stm_set_active / stm_set_active_auto, include/stm_hip.h): mode 0 = off (not one launch changes), 1 = a
// given rectangle, 2 = measured on each frame's left eye on the device.  The depth fit and the overlay fit of a frame call read the
// rectangle on the device; with `fill` the maps handed back take fill_disp outside it.  One per host thread, next to the cut
// detector; a frame stream installs its own copy around its frame calls.
struct Active {
    int mode;
    int rect[4];        // mode 1: {top, bottom, left, right}, rows [top, bottom) and columns [left, right)
    int fill;
    float fill_disp;
    int thresh_luma, lit_permille, max_bar_permille, hold; // mode 2
    int *d_state;       // mode 2: the 16 ints of stm_active_detect in device memory; null = scratch, every frame on its own
};
Active active_default();
Active active();
void set_active(const Active &a);
// the argument rules of the two settings; false with the error recorded
bool active_params_ok(const char *fn, int mode, const int *rect, int fill, float fill_disp);
bool active_auto_params_ok(const char *fn, int thresh_luma, int lit_permille, int max_bar_permille, int hold);
// the measurement's frame rule: num_rows * num_cols < 2^31; false with the error recorded
bool active_size_ok(const char *fn, int num_rows, int num_cols);
// a rectangle against a map: 0 <= top < bottom <= num_rows and 0 <= left < right <= num_cols; false with the error recorded
bool active_rect_ok(const char *fn, const int *rect, int num_rows, int num_cols);
constexpr size_t ACTIVE_STATE_WORDS = 16;
// the measurement (stm_kernels_active.hip) on the left eye of a screened frame (in != nullptr) or on one unpacked image
// H x W x elem_sz: the lit pixels per row and column into counts (H + W words), the decision and the update of `state` (16 ints);
// restart: the state's history is ignored; cut_state: the shot-change detector's state or null
void launch_active_detect(int *state, uint32_t *counts, const PackInput *in, const u8 *img_l, int H, int W, int elem_sz, int thresh_luma,
                          int lit_permille, int max_bar_permille, int hold, bool restart, const int *cut_state);
// a given rectangle's four words written to d_rect by a kernel (no copy node, nothing the host must keep alive)
void launch_active_rect(int *d_rect, const int rect[4]);
// disp[i] (H x W), i < nmaps (1 or 2), takes `value` outside the rectangle d_rect holds; one launch over the four strips
void launch_active_fill(int nmaps, float *const *disp, int H, int W, const int *d_rect, float value);
// The test tap on the frame's aggregation chain (stm_set_agg_tap, include/stm_hip.h): the caller's float [2][D][H][W] buffers that
// receive the volume after the first horizontal pass (h1), after both vertical passes (v2) and after a last pass that keeps its
// volume (h4), and the volume written over V2 before the last pass (inject_v2).  All null = off: not one launch changes.  One per
// host thread; a frame stream switches it off around its frame calls (a captured graph must not hold the copies).
struct AggTap {
    float *h1, *v2, *h4;
    const float *inject_v2;
    bool on() const { return h1 || v2 || h4 || inject_v2; }
};
AggTap agg_tap();
void set_agg_tap(const AggTap &t);
// the copies (stm_kernels_aggtap.hip) between one volume per view in a layout of the chain and a tap buffer, on the launch stream.
// ord: the hypothesis order of a PX record (px_order, stm_kernels_aggm.hip).  launch_tap_write also sets the padding hypotheses
// d >= D of the layout's last chunk to -1.0f
enum { TAP_PQ = 0, TAP_PX = 1, TAP_QUADS = 2 };
void launch_tap_read(const float *vol_l, const float *vol_r, int layout, int ord, float *dst, int D, int H, int W);
void launch_tap_write(float *vol_l, float *vol_r, int layout, int ord, const float *src, int D, int H, int W);
// aggregation on the matrix pipe (stm_kernels_aggm.hip): the frame pipeline's cost -> H -> V, V -> H + WTA
struct PQViews { // both views of a frame; a / b = the two PQ volumes of a view
    const uint32_t *pk[2], *cen[2];
    float *a[2], *b[2];
    const u8 *armU[2], *armD[2], *armL[2], *armR[2];
    float *disp[2];
};
size_t pq_volume_floats(int D, int H, int W);
bool aggm_supports(int usd, int H, int W);
void launch_aggm_frame(const uint32_t *const *pk, const uint32_t *const *cen, const float *lut, float *const *vol_a, float *const *vol_b,
                       const u8 *const *armU, const u8 *const *armD, const u8 *const *armL, const u8 *const *armR, float *const *disp,
                       int D, int zd, int H, int W, int usd, bool keep_volume = false, uint32_t *htab_ready = nullptr, uint32_t *vtab_ready = nullptr,
                       bool v2_read_later = false); // v2_read_later: a later stage reads vol_a as a PQ volume (no PX layout)
size_t aggm_frame_htab_dwords(int D, int H, int W, int usd, bool keep_volume);
// the vertical table in a register-ring kernel's static layout, or 0; *col: the per-column layout of the PX fast path (aggm_frame_px)
size_t aggm_frame_vtab_dwords(int D, int zd, int H, int W, int usd, bool keep_volume, bool v2_read_later, int *rec, int *top, bool *col);
// whether the frame's two intermediate volumes take the pixel-major layout PX (float index ((y 4G + x) 64 + d), DESIGN.md
// section 4): all three register / streaming kernels run, 48 < D <= 64, WTA, and nobody reads a volume afterwards
bool aggm_frame_px(int D, int zd, int H, int W, int usd, bool keep_volume, bool v2_read_later);
// the order of the hypotheses inside a PX pixel's record as the last pass reads it where aggm_frame_px holds (0: d at float d;
// 2: 4 n + b at float 16 b + n, after the 16-byte stores of the first pass and of stm_k_pq_v12r), else -1
int aggm_frame_px_order(int D, int zd, int H, int W, int usd, bool keep_volume, bool v2_read_later);
// what launch_aggm_frame runs for these arguments, as the bits 1 .. 16 of stm_agg_path (include/stm_hip.h); launches nothing
int aggm_frame_path(int D, int zd, int H, int W, int usd, bool keep_volume, bool v2_read_later);
// the blocks per image row of stm_k_pq_hc2 (first pass, both views from one ring of costs) where launch_aggm_frame runs it, else 0
int aggm_frame_hc2_parts(int D, int zd, int H, int W, int usd, bool keep_volume, bool v2_read_later);
// ca_cross / d_ca_cross of one volume in the caller's layout on the matrix-pipe kernels; `out` may be `in`.  Returns false, with
// `out` untouched, when the volume holds an infinite, NaN or denormal element (one host read-back of a flag): the caller runs
// the vector-ALU kernels instead.  aggm_stage_bytes: what it carves from the current Workspace scope.
bool launch_aggm_stage(Vol in, Vol out, const u8 *armU, const u8 *armD, const u8 *armL, const u8 *armR, int D, int H, int W, int usd);
size_t aggm_stage_bytes(int D, int H, int W, int usd);
// both vertical passes with a strip's rows in registers (stm_kernels_aggv.hip); `tab` / `rec`: the table of stm_k_vwin_table
bool aggh_supports(int usd, int D); // stm_kernels_aggh.hip: last horizontal pass + WTA with the row's window range in registers
size_t aggh_table_dwords(int nviews, int H, int W);
void launch_hwin_table(PQViews &v, int nviews, uint32_t *tab, int H, int W); // (the frame path builds the table inside stm_k_cross_arms: launch_cross_arms2's htab)
void launch_pq_hsr(PQViews &v, int nviews, const uint32_t *tab, int D, int zd, int H, int W, bool px = false, int ord = 0); // px: vol_a in the PX layout, its records in hypothesis order ord
bool aggv_supports(int usd);
int aggv_table_top();
int aggv_table_rec();
void launch_pq_v12q(PQViews &v, int nviews, const uint32_t *tab, int rec, int H, int W, int G, int NC); // PQ volumes, a strip of four columns per wave
void launch_pq_v12r(PQViews &v, int nviews, const uint32_t *tab, int H, int W, int G, bool x4 = false); // PX volumes, one column per wave; tab: the per-column table; x4: records leave in order 2
void launch_vcol_table(PQViews &v, int nviews, uint32_t *tab, int H, int W);                            // that table from the arm planes (aggv_col_table_dwords)
size_t aggv_col_table_dwords(int nviews, int H, int W);
bool aggv_col_vadd(); // that table holds the arms as jump offsets (stm_k_pq_v12r, the default), not mask records (stm_k_pq_v12m, stm_set_agg_variant(800))
void launch_to_pq(Vol in, float *pq, int D, int H, int W, uint32_t *odd = nullptr); // stm_kernels_hslo.hip; odd: see stm_k_to_pq
void launch_from_pq(const float *pq, Vol out, int D, int H, int W); // stm_kernels_aggm.hip
// HSLO (stm_kernels_hslo.hip)
void launch_hslo_wta(int nviews, const Vol *cost, const u8 *const *img_a, const u8 *const *img_b, const int *osign,
                     float *const *disp, float T, float H1, float H2, int D, int zd, int H, int W, int elem_sz);
// The test tap on the scanline passes (stm_set_hslo_tap, include/stm_hslo_tap.h): the caller's float [views][D][H][W] buffers that
// receive the accumulator after the horizontal passes (s2 = C_lr + C_rl), after the top-to-bottom pass (s3 = s2 + C_tb) and the final
// volume (fin = (s3 + C_bt) * 0.25f), image columns only; views = the nviews of the run.  All null = off: not one launch is added.
// One per host thread; a frame stream refuses stage bit 0x100, so its frames never run the tap.
struct HsloTap {
    float *s2, *s3, *fin;
};
HsloTap hslo_tap();
void set_hslo_tap(const HsloTap &t);
// the same on PQ volumes (the frame pipeline): cost_pq read only, acc_pq scratch of the same size
void launch_hslo_wta_pq(int nviews, float *const *cost_pq, float *const *acc_pq, const u8 *const *img_a, const u8 *const *img_b,
                        const int *osign, float *const *disp, float T, float H1, float H2, int D, int zd, int H, int W, int elem_sz);

// host-built tables (same formulas as the reference's host code; see stm_tables.cpp)
void rho_luts(float ad_coeff, float census_coeff, float *lut_ad /*766*/, float *lut_census /*65*/);
void gaussian_kernel_2d(float *kernel, int radius, float sigma);
void gaussian_kernel_1d(float *kernel, int size, float sigma);
float mux_y_interval(int num_views, float angle, int elem_sz);

} // namespace stm
