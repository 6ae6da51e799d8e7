// stm_stream.hip -- pipelined side-by-side frame sequence processor.
//
// The reference's video loop (video_io.cpp:144-165) calls adcensus_stm once per decoded frame; every call
// uploads the frame, computes, downloads three results and only then returns, so PCIe transfers and compute
// never overlap.  This front end keeps the same per-frame contract (one SBS frame in; disp_l, disp_r and the
// interlaced frame out, in submission order) but runs an upload stream, a download stream and one COMPUTE stream +
// private workspace per buffer slot over double-buffered pinned / device buffers: while frame k computes, frame k+1 is
// uploading and frame k-1 is downloading, and (round 3) the two frames in flight also overlap ON the GPU: the
// latency-bound tail of frame k (region voting, filters, view synthesis) shares the chip with the issue-bound aggregation
// of frame k+1 (bench.py's rate_two_in_flight measures that overlap for device-resident frames).  STM_STREAM_OVERLAP=0: one
// compute stream and workspace for both slots, as in round 2.
#include "stm_common.h"
#include "../../include/stm_hip.h"
#include "../../include/stm_depth_input.h"
#include "../../include/stm_depth_video.h"
#include "../../include/stm_rectify.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace {

struct Slot {
    u8 *h_in = nullptr, *d_in = nullptr, *d_out = nullptr, *h_out = nullptr;
    float *d_dl = nullptr, *d_dr = nullptr, *h_dl = nullptr, *h_dr = nullptr; // (h_dl, h_dr: null while stm_stream_maps' format is not 0)
    u8 *d_pl = nullptr, *h_pl = nullptr; // stm_stream_maps, formats 2 and 3: the slot's planes, tight behind each other, and their download
    u8 *d_img_l = nullptr, *d_img_r = nullptr; // NV12 input: the slot's converted split images (the other slot's frame reads them as its history)
    float *d_rec = nullptr, *h_rec = nullptr; // depth mode 2: the state as this slot's frame left it (16 bytes), and its download
    float *d_arec = nullptr, *h_arec = nullptr; // align mode 2: likewise the alignment's state
    int *d_brec = nullptr, *h_brec = nullptr;   // balance mode 2: likewise the balance's state (769 ints)
    int *d_crec = nullptr, *h_crec = nullptr;   // cut mode 1: {cut, since, score} as this slot's frame's decision left them (12 bytes)
    int *d_acrec = nullptr, *h_acrec = nullptr; // active mode 2: {top, bottom, left, right, changed} as this slot's frame left them (20 bytes)
    u8 *h_ov = nullptr, *d_ov = nullptr;      // stm_stream_set_overlay: the slot's pinned and device copy of the overlay's pixels
    long ov_gen = 0;                          // ... and which stm_stream_overlay call they hold (0 = none yet)
    float *d_orec = nullptr, *h_orec = nullptr; // stm_stream_set_overlay_auto: the overlay's state as this slot's frame left it (16 bytes), and its download
    float ov_disparity = 0.0f;                // the setter's disparity this slot's frame was submitted under (0 without an overlay)
    hipEvent_t ev_in, ev_done, ev_out;
    bool busy = false;
    hipStream_t s_compute = nullptr; // this slot's compute stream and private workspace (shared by both slots when overlap is off)
    void *ws = nullptr;              // private: the addresses baked into the slot's graph stay valid
    // the slot's frame pipeline as a captured graph: a frame is ~30 launches with fixed arguments (the slot's buffers,
    // the stream's private workspace), replayed with one hipGraphLaunch
    hipGraphExec_t gexec = nullptr;
    void *g_ws_base = nullptr;
    size_t g_ws_cap = 0;
    int eager_runs = 0;
};

struct FrameStream {
    int H, Wsbs, W, Hout, Wout, E, N, D, zd, usd, lsd, thresh_s;
    float angle, ad, ce, ucd, lcd, thresh_h;
    size_t in_sz, out_sz, hw;
    int dev = 0; // the device the stream was created on: submit / collect switch to it (and back) if the caller's differs
    hipStream_t s_in, s_out;
    bool overlap = true; // two frames in flight on the GPU (a compute stream + workspace per slot)
    bool use_graph = true;
    int stages = 3; // stm_stream_set_stages: 3, optionally with 0x200 / 0x400 / 0x800 / 0x2000 (and 0x1000 with a match size)
    float t_alpha = 0.5f, t_disp = 1.5f; // stm_stream_set_temporal: the parameters of the temporal step (0x2000) and their defaults
    int t_color = 24;
    int in_format = 0, in_matrix = 0; // stm_stream_set_input: 0 = side-by-side BGR, 1 = NV12 (Y plane, then the UV plane; pitch Wsbs)
    size_t in_bytes = 0;              // what a submit copies and uploads: in_sz, or H * Wsbs * 3 / 2 for NV12
    stm::Lens lens = {0, 0.0, 0.0, 0.0}; // stm_stream_set_lens: the stream's own display geometry, installed around its frame calls
    stm::Layout layout = {0, 1, 1, 0, 0}; // stm_stream_set_layout: the stream's own output geometry, installed around its frame calls
    stm::Output output = {0, 0, 0, 0};    // stm_stream_set_output: the stream's own output format, installed around its frame calls
    size_t out_bytes = 0;                 // what a collect copies and the download moves: out_sz, or Hout * Wout * 3 / 2 for NV12
    stm::Depth depth = {0, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 20, nullptr}; // stm_stream_set_depth / _auto: the stream's own depth budget
    stm::Packing packing = {0, 0, 0, 0}; // stm_stream_set_packing: the stream's own input packing, installed around its frame calls
    int rows_f = 0;                      // the rows of an input frame: H, or what the packing makes of it
    int match_h = 0, match_w = 0;        // stm_stream_set_match_size: the size the pair is matched at (0, 0 = off: the full-resolution frame)
    float match_scale = 1.0f;            // ... and the reduced frame's disp_scale
    stm::Antialias antialias = {0, 0.0f, 0, 0.0f}; // stm_stream_set_antialias: the stream's own view antialiasing
    float *d_depth_state = nullptr; // mode 2: the state every frame updates, at one address for both slots' graphs
    stm::Align align = {0, 0.0f, 0.0f, 0.0f, 16, 1.0f, nullptr}; // stm_stream_set_align / _auto: the stream's own vertical alignment
    float *d_align_state = nullptr; // align mode 2: the state every frame updates, at one address for both slots' graphs
    stm::Balance balance = stm::balance_default(); // stm_stream_set_balance / _auto: the stream's own colour balance
    int *d_balance_state = nullptr; // balance mode 2: the state every frame updates, at one address for both slots' graphs
    stm::Cut cut = stm::cut_default(); // stm_stream_set_cut: the stream's own shot-change detector
    int *d_cut_state = nullptr;     // cut mode 1: the 260 ints every frame updates, at one address for both slots' graphs
    stm::Active active = stm::active_default(); // stm_stream_set_active: the stream's own active picture area
    int *d_active_state = nullptr;  // active mode 1 and 2: 16 ints at one address for both slots' graphs; mode 2 updates them on every
                                    // frame, mode 1 wrote the given rectangle into words 1 .. 4 once (the overlay fit behind the graph reads it)
    int ov_max_rows = 0, ov_max_cols = 0; // stm_stream_set_overlay: the largest overlay the slots' copies hold ((0, 0) = off)
    u8 *ov_pixels = nullptr;              // stm_stream_overlay: the pixels of the overlay in force (host memory of the stream's own)
    stm::Overlay ov = {0, nullptr, 0, 0, 0, 0, 0.0f}; // ... and its arguments; mode 0 = none.  d_overlay is filled in per slot
    long ov_gen = 0;                      // counts the stm_stream_overlay calls that brought pixels
    stm::OverlayAuto ov_auto = stm::overlay_auto_default(); // stm_stream_set_overlay_auto: the stream's own automatic placement
    float *d_ov_state = nullptr;          // ... its state {valid, disparity, nearest, 0}, at one address for every frame
    uint32_t *d_ov_ws = nullptr;          // ... and the fit's bins and alpha box
    long ov_fit_gen = 0;                  // the overlay generation the last fitted frame was submitted under
    int maps_format = 0, maps_which = 2; // stm_stream_maps: what a frame's maps leave as (0 = float32, 1 = not at all, 2 = u8, 3 = u16 planes)
    float maps_lo = 0.0f, maps_k = 0.0f; // ... formats 2 and 3: the definition's lo and k
    size_t plane_bytes = 0;              // ... the bytes of one plane
    int planes = 0;                      // ... and how many a frame has (which 2: left, then right)
    stm::DepthInput din = {-1, 0.0f, 0.0f, 0, 0.0f}; // stm_stream_input_depth: a frame is an image and its depth plane (format -1 = off)
    size_t plane_off = 0;                // ... the plane's byte offset in a frame: the image's bytes rounded up to a multiple of 16
    stm::DepthVideo dvid = {-1, 0, {0, 0, 0, 0}, 0, 0, 0, 0.0f, 0.0f, 0, 0.0f}; // stm_stream_input_packed_depth: a frame is one packed BGR or
                                         // NV12 picture, the image in one half and its depth in the other (format -1 = off)
    stm::Rectify rectify = {0, {{0.0f}, {0.0f}}, 0}; // stm_stream_rectify: the stream's own rectification, installed around its frame calls
    Slot slot[2];
    long submitted = 0, collected = 0;
};

// the stream's geometry in place of the calling thread's for the duration of a submit
struct LensScope {
    stm::Lens saved;
    explicit LensScope(const stm::Lens &l) : saved(stm::lens()) { stm::set_lens(l); }
    ~LensScope() { stm::set_lens(saved); }
};

struct LayoutScope {
    stm::Layout saved;
    explicit LayoutScope(const stm::Layout &l) : saved(stm::layout()) { stm::set_layout(l); }
    ~LayoutScope() { stm::set_layout(saved); }
};

struct OutputScope {
    stm::Output saved;
    explicit OutputScope(const stm::Output &o) : saved(stm::output()) { stm::set_output(o); }
    ~OutputScope() { stm::set_output(saved); }
};

struct DepthScope {
    stm::Depth saved;
    explicit DepthScope(const stm::Depth &d) : saved(stm::depth()) { stm::set_depth(d); }
    ~DepthScope() { stm::set_depth(saved); }
};

struct AlignScope {
    stm::Align saved;
    explicit AlignScope(const stm::Align &a) : saved(stm::align()) { stm::set_align(a); }
    ~AlignScope() { stm::set_align(saved); }
};

struct RectifyScope {
    stm::Rectify saved;
    explicit RectifyScope(const stm::Rectify &r) : saved(stm::rectify()) { stm::set_rectify(r); }
    ~RectifyScope() { stm::set_rectify(saved); }
};

struct BalanceScope {
    stm::Balance saved;
    explicit BalanceScope(const stm::Balance &b) : saved(stm::balance()) { stm::set_balance(b); }
    ~BalanceScope() { stm::set_balance(saved); }
};

struct ActiveScope {
    stm::Active saved;
    explicit ActiveScope(const stm::Active &a) : saved(stm::active()) { stm::set_active(a); }
    ~ActiveScope() { stm::set_active(saved); }
};
struct CutScope {
    stm::Cut saved;
    explicit CutScope(const stm::Cut &c) : saved(stm::cut()) { stm::set_cut(c); }
    ~CutScope() { stm::set_cut(saved); }
};

struct AntialiasScope {
    stm::Antialias saved;
    explicit AntialiasScope(const stm::Antialias &a) : saved(stm::antialias()) { stm::set_antialias(a); }
    ~AntialiasScope() { stm::set_antialias(saved); }
};

// the calling thread's overlay (stm_set_overlay) never reaches a stream's frames: the stream composites its own after the frame call
struct OverlayOffScope {
    stm::Overlay saved;
    OverlayOffScope() : saved(stm::overlay()) { stm::set_overlay(stm::Overlay{0, nullptr, 0, 0, 0, 0, 0.0f}); }
    ~OverlayOffScope() { stm::set_overlay(saved); }
};
// nor does the thread's test tap on the aggregation chain (stm_set_agg_tap): a captured graph must not hold its copies
struct AggTapOffScope {
    stm::AggTap saved;
    AggTapOffScope() : saved(stm::agg_tap()) { stm::set_agg_tap(stm::AggTap{nullptr, nullptr, nullptr, nullptr}); }
    ~AggTapOffScope() { stm::set_agg_tap(saved); }
};

struct PackingScope {
    stm::Packing saved;
    explicit PackingScope(const stm::Packing &p) : saved(stm::packing()) { stm::set_packing(p); }
    ~PackingScope() { stm::set_packing(saved); }
};

// the rules an input format and a packing set together on the stream's geometry (either may come first); false with the error recorded
bool stream_input_ok(const char *fn, const FrameStream *f, int format, int matrix, const stm::Packing &pk)
{
    if (format == 1 && (f->Wsbs & 1)) // the UV plane follows the Y plane with the same pitch
        return STM_REJECT("num_cols_sbs", "%s: NV12 needs an even num_cols_sbs", fn);
    if (pk.on()) return stm::packing_args_ok(fn, pk, f->H, f->Wsbs, f->W, "num_cols", format == 1, f->Wsbs, f->Wsbs, matrix);
    return format != 1 || stm::nv12_args_ok(fn, f->H, f->Wsbs, f->W, "num_cols", f->Wsbs, f->Wsbs, matrix);
}
// what the slots' graphs capture is set before the first submit only; false with the error recorded
bool not_submitted(const FrameStream *f, const char *fn, const char *arg = "stream")
{
    return f->submitted == 0 || STM_REJECT(arg, "%s: only before the first submit", fn);
}
// the settings that condition a stereo pair or its matcher do not go with image-plus-depth frames (stm_stream_input_depth); false with
// the error recorded
bool no_depth_input(const FrameStream *f, const char *fn, const char *arg)
{
    return f->din.format < 0 || STM_REJECT(arg, "%s: the stream has depth input (stm_stream_input_depth): a frame is an image and its depth plane, "
                                           "nothing is matched and there is no second image to condition; switch the depth input off first", fn);
}
// likewise with packed 2D-plus-depth video frames (stm_stream_input_packed_depth): the frame's format and packing are that call's own
bool no_depth_video(const FrameStream *f, const char *fn, const char *arg)
{
    return f->dvid.format < 0 || STM_REJECT(arg, "%s: the stream has packed depth video input (stm_stream_input_packed_depth): a frame is an image and "
                                            "its depth picture in one packed frame whose format and packing that call sets, and nothing is matched; "
                                            "switch it off first", fn);
}
// stm_stream_collect / _view on a stream that downloads no float maps (stm_stream_maps, format != 0): a map pointer has nothing to
// receive.  false with the error recorded; the caller consumes nothing
bool float_maps_ok(const FrameStream *f, const char *fn, const void *disp_l, const void *disp_r)
{
    if (f->maps_format == 0 || (!disp_l && !disp_r)) return true;
    stm::clear_failed();
    return STM_REJECT("disp_l, disp_r", "%s: the stream's maps format is %d (stm_stream_maps): it downloads no float maps, disp_l and disp_r must "
                      "be null (the planes: stm_stream_collect_maps)", fn, f->maps_format);
}
// stm_stream_collect_maps / _view: not on a stream of float maps, and no destination for a plane the stream does not produce
bool planes_ok(const FrameStream *f, const char *fn, const void *plane_l, const void *plane_r)
{
    if (f->maps_format == 0) {
        stm::clear_failed();
        return STM_REJECT("stream", "%s: the stream's maps format is 0 (float32 maps): stm_stream_collect hands them out; planes need "
                          "stm_stream_maps before the first submit", fn);
    }
    const bool left = f->planes > 0 && f->maps_which != 1, right = f->planes > 0 && f->maps_which != 0;
    if ((plane_l && !left) || (plane_r && !right)) {
        stm::clear_failed();
        return STM_REJECT(plane_l && !left ? "plane_l" : "plane_r", "%s: the stream produces no %s plane (stm_stream_maps: format %d, which %d): "
                          "its pointer must be null", fn, plane_l && !left ? "left" : "right", f->maps_format, f->maps_which);
    }
    return true;
}

} // namespace

extern "C" {

void *stm_stream_create(int num_rows, int num_cols_sbs, int num_cols, int num_rows_out, int num_cols_out, int elem_sz,
                        int num_views, float angle, int num_disp, int zero_disp, float ad_coeff, float census_coeff,
                        float ucd, float lcd, int usd, int lsd, int thresh_s, float thresh_h)
{
    FrameStream *f = new FrameStream();
    f->H = num_rows; f->Wsbs = num_cols_sbs; f->W = num_cols; f->Hout = num_rows_out; f->Wout = num_cols_out; f->E = elem_sz;
    f->N = num_views; f->angle = angle; f->D = num_disp; f->zd = zero_disp; f->ad = ad_coeff; f->ce = census_coeff;
    f->ucd = ucd; f->lcd = lcd; f->usd = usd; f->lsd = lsd; f->thresh_s = thresh_s; f->thresh_h = thresh_h;
    f->in_sz = (size_t)num_rows * num_cols_sbs * elem_sz;
    f->in_bytes = f->in_sz;
    f->rows_f = num_rows;
    f->out_sz = (size_t)num_rows_out * num_cols_out * elem_sz;
    f->out_bytes = f->out_sz;
    f->hw = (size_t)num_rows * num_cols;
    STM_CHECK(hipGetDevice(&f->dev));
    STM_CHECK(hipStreamCreateWithFlags(&f->s_in, hipStreamNonBlocking));
    STM_CHECK(hipStreamCreateWithFlags(&f->s_out, hipStreamNonBlocking));
    const char *g = getenv("STM_STREAM_GRAPH"); // STM_STREAM_GRAPH=0: always launch kernel by kernel
    f->use_graph = !(g && g[0] == '0');
    const char *o = getenv("STM_STREAM_OVERLAP"); // STM_STREAM_OVERLAP=0: one compute stream + workspace for both slots
    f->overlap = !(o && o[0] == '0');
    for (int i = 0; i < 2; ++i) {
        Slot &s = f->slot[i];
        if (i == 0 || f->overlap) {
            STM_CHECK(hipStreamCreateWithFlags(&s.s_compute, hipStreamNonBlocking));
            s.ws = stm::ws_private_create();
        } else {
            s.s_compute = f->slot[0].s_compute;
            s.ws = f->slot[0].ws;
        }
        STM_CHECK(hipHostMalloc((void **)&s.h_in, f->in_sz, hipHostMallocDefault));
        STM_CHECK(hipHostMalloc((void **)&s.h_out, f->out_sz, hipHostMallocDefault));
        STM_CHECK(hipHostMalloc((void **)&s.h_dl, f->hw * 4, hipHostMallocDefault));
        STM_CHECK(hipHostMalloc((void **)&s.h_dr, f->hw * 4, hipHostMallocDefault));
        STM_CHECK(hipMalloc((void **)&s.d_in, f->in_sz));
        STM_CHECK(hipMalloc((void **)&s.d_out, f->out_sz));
        STM_CHECK(hipMalloc((void **)&s.d_dl, f->hw * 4));
        STM_CHECK(hipMalloc((void **)&s.d_dr, f->hw * 4));
        STM_CHECK(hipMemsetAsync(s.d_out, 0, f->out_sz, s.s_compute)); // ordered before the first frame's writes
        STM_CHECK(hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming));
        STM_CHECK(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
        STM_CHECK(hipEventCreateWithFlags(&s.ev_out, hipEventDisableTiming));
    }
    return f;
}

// The `stages` word every frame of the stream is computed with: 3 (the default), optionally OR-ed with 0x200 (sub-pixel), 0x400
// (outlier interpolation), 0x800 (linear sampling of the warps) and / or 0x2000 (temporal stabilisation: every frame but the first
// is computed by stm_d_adcensus_stm_t with the frame before it as its history).  Not 0x100: the stream's workspace is sized for
// the frame without HSLO.  Only before the first submit: afterwards the slots replay their launches from a captured graph.
// Returns 0, or -1 with the error recorded.
int stm_stream_set_stages(void *h, int stages)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    const bool reduced = f->match_h > 0;
    if ((stages & 0x1000) && !reduced) // the stream runs the full-resolution frame: nothing is up-scaled
        return STM_REJECT("stages", "stream_set_stages: stages 0x1000 (guided disparity up-sampling) needs the reduced-resolution frame") ? 0 : -1;
    if ((stages & ~(reduced ? 0x3e00 : 0x2e00)) != 3)
        return STM_REJECT("stages", "stream_set_stages: stages must be 3, optionally OR-ed with 0x200, 0x400, 0x800%s and 0x2000",
                          reduced ? ", 0x1000" : "") ? 0 : -1;
    if ((stages & ~0x800) != 3 && !no_depth_input(f, "stream_set_stages", "stages")) return -1; // 3 and 3 | 0x800 render only
    if ((stages & ~0x800) != 3 && !no_depth_video(f, "stream_set_stages", "stages")) return -1;
    if (!not_submitted(f, "stream_set_stages", "stages")) return -1;
    f->stages = stages;
    return 0;
}

// The size every frame of the stream is matched at (stm_hip.h): with a size set, a frame is the reduced-resolution frame
// (stm_d_adcensus_stm_2s, _2t with stages bit 0x2000, _2nv12 in NV12 mode) and stm_stream_set_stages also takes 0x1000.  (0, 0, any)
// = off, the default.  Not together with a packing of the stream, and not switched off while the stream's stages hold 0x1000.  Only
// before the first submit.  Returns 0, or -1 with the error recorded.
int stm_stream_set_match_size(void *h, int num_rows_disp, int num_cols_disp, float disp_scale)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    const bool off = num_rows_disp == 0 && num_cols_disp == 0;
    if (!off && (num_rows_disp < 1 || num_cols_disp < 1))
        return STM_REJECT("num_rows_disp, num_cols_disp", "stream_set_match_size: num_rows_disp and num_cols_disp must be >= 1, or both 0 (off)") ? 0 : -1;
    if (!off && !(disp_scale > 0.0f && disp_scale <= 3.402823466e38f)) // (NaN fails the first comparison)
        return STM_REJECT("disp_scale", "stream_set_match_size: disp_scale must be finite and > 0") ? 0 : -1;
    if (!no_depth_input(f, "stream_set_match_size", "stream")) return -1;
    if (!no_depth_video(f, "stream_set_match_size", "stream")) return -1;
    if (!not_submitted(f, "stream_set_match_size")) return -1;
    if (!off && f->packing.on())
        return STM_REJECT("packing", "stream_set_match_size: the stream has a packing (stm_stream_set_packing), which the reduced-resolution frame "
                          "does not support") ? 0 : -1;
    if (off && (f->stages & 0x1000))
        return STM_REJECT("stages", "stream_set_match_size: the stream's stages hold 0x1000 (guided disparity up-sampling), which needs a match size")
                   ? 0 : -1;
    f->match_h = off ? 0 : num_rows_disp;
    f->match_w = off ? 0 : num_cols_disp;
    f->match_scale = off ? 1.0f : disp_scale;
    return 0;
}

// The parameters of the temporal step (stages bit 0x2000; stm_disp_temporal's rules): defaults 0.5, 24, 1.5.  Only before the
// first submit.  Returns 0, or -1 with the error recorded.
int stm_stream_set_temporal(void *h, float alpha, int thresh_color, float thresh_disp)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (!(alpha >= 0.0f && alpha <= 1.0f)) return STM_REJECT("alpha", "stream_set_temporal: alpha must be in [0, 1]") ? 0 : -1;
    if (thresh_color < 0 || thresh_color > 765) return STM_REJECT("thresh_color", "stream_set_temporal: thresh_color must be in [0, 765]") ? 0 : -1;
    if (!(thresh_disp >= 0.0f)) return STM_REJECT("thresh_disp", "stream_set_temporal: thresh_disp must be >= 0") ? 0 : -1;
    if (!not_submitted(f, "stream_set_temporal")) return -1;
    f->t_alpha = alpha; f->t_color = thresh_color; f->t_disp = thresh_disp;
    return 0;
}

// The input format of the stream's frames (stm_hip.h): 0 = BGR, 1 = NV12 with `matrix`.  The slots' input buffers, sized for a BGR
// frame, hold the NV12 frame's two planes; the split images a slot's frames convert into are allocated here.  Only before the first
// submit.  Returns 0, or -1 with the error recorded.
int stm_stream_set_input(void *h, int format, int matrix)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (format != 0 && format != 1) return STM_REJECT("format", "stream_set_input: format must be 0 (side-by-side BGR) or 1 (NV12)") ? 0 : -1;
    if (!no_depth_input(f, "stream_set_input", "stream")) return -1;
    if (!no_depth_video(f, "stream_set_input", "stream")) return -1;
    if (!not_submitted(f, "stream_set_input")) return -1;
    if (format == 1) {
        if (!stream_input_ok("stream_set_input", f, format, matrix, f->packing)) return -1;
        for (Slot &s : f->slot)
            if (!s.d_img_l) {
                STM_CHECK(hipMalloc((void **)&s.d_img_l, f->hw * f->E));
                STM_CHECK(hipMalloc((void **)&s.d_img_r, f->hw * f->E));
            }
        if (stm::failed()) return -1;
    }
    f->in_format = format;
    f->in_matrix = format == 1 ? matrix : 0;
    f->in_bytes = format == 1 ? (size_t)f->rows_f * f->Wsbs * 3 / 2 : f->in_sz;
    return 0;
}

// The packing of the stream's input frames (stm_hip.h; stm_set_packing's settings and the geometry rules of stm_demux_packed, or of
// stm_demux_nv12_packed in NV12 mode, on the stream's num_rows, num_cols_sbs and num_cols).  A packed frame has rows_f rows, so each
// slot's pinned and device input buffers are allocated anew for rows_f * num_cols_sbs * elem_sz bytes: pointers handed out by
// stm_stream_input_buffer before this call are void.  Kept and installed like the lens geometry.  Only before the first submit.
// Returns 0, or -1 with the error recorded.
int stm_stream_set_packing(void *h, int packing, int swap, int filter, int gap)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    const stm::Packing pk = {packing, swap, filter, gap};
    if (!stm::packing_params_ok("stream_set_packing", pk)) return -1;
    if (!no_depth_input(f, "stream_set_packing", "stream")) return -1;
    if (!no_depth_video(f, "stream_set_packing", "stream")) return -1;
    if (!not_submitted(f, "stream_set_packing")) return -1;
    if (pk.on() && f->match_h > 0)
        return STM_REJECT("packing", "stream_set_packing: the stream has a match size (stm_stream_set_match_size): the reduced-resolution frame "
                          "takes no packing") ? 0 : -1;
    if (!stream_input_ok("stream_set_packing", f, f->in_format, f->in_matrix, pk)) return -1;
    const int rows_f = pk.rows_f(f->H);
    const size_t in_sz = (size_t)rows_f * f->Wsbs * f->E;
    if (in_sz != f->in_sz) {
        int caller_dev = f->dev;
        STM_CHECK(hipGetDevice(&caller_dev));
        if (caller_dev != f->dev) STM_CHECK(hipSetDevice(f->dev));
        // the new buffers first, the old ones freed only once all four exist: a failed allocation leaves the stream as it was
        u8 *h_new[2] = {nullptr, nullptr}, *d_new[2] = {nullptr, nullptr};
        for (int i = 0; i < 2; ++i) {
            STM_CHECK(hipHostMalloc((void **)&h_new[i], in_sz, hipHostMallocDefault));
            STM_CHECK(hipMalloc((void **)&d_new[i], in_sz));
        }
        if (stm::failed()) { // (error mode 1; the hip calls take null pointers)
            for (int i = 0; i < 2; ++i) {
                if (h_new[i]) (void)hipHostFree(h_new[i]);
                if (d_new[i]) (void)hipFree(d_new[i]);
            }
            if (caller_dev != f->dev) (void)hipSetDevice(caller_dev);
            return -1;
        }
        for (int i = 0; i < 2; ++i) {
            Slot &s = f->slot[i];
            STM_CHECK(hipHostFree(s.h_in));
            STM_CHECK(hipFree(s.d_in));
            s.h_in = h_new[i];
            s.d_in = d_new[i];
        }
        if (caller_dev != f->dev) STM_CHECK(hipSetDevice(caller_dev));
    }
    f->packing = pk;
    f->rows_f = rows_f;
    f->in_sz = in_sz;
    f->in_bytes = f->in_format == 1 ? (size_t)rows_f * f->Wsbs * 3 / 2 : in_sz;
    return 0;
}

// The display geometry every frame of the stream is interlaced through (stm_set_lens's rules; the default is mode 0, the reference's
// interlacer).  The stream keeps its own copy: a submit installs it for its frame call and puts the calling thread's setting back,
// so neither changes the other.  Only before the first submit: afterwards the slots replay their launches from a captured graph.
// Returns 0, or -1 with the error recorded.
int stm_stream_set_lens(void *h, int mode, double pitch, double slope, double centre)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (!stm::lens_params_ok("stream_set_lens", mode, 0, 3, pitch, slope, centre)) return -1;
    if (!not_submitted(f, "stream_set_lens")) return -1;
    f->lens = mode == 0 ? stm::Lens{0, 0.0, 0.0, 0.0} : stm::Lens{mode, pitch, slope, centre};
    return 0;
}

// The output geometry of every frame of the stream (stm_set_layout's rules; the default is layout 0, the interlaced frame).  Kept and
// installed like the lens geometry; the tiling is screened against the stream's geometry by the first frame call.  Only before the
// first submit.  Returns 0, or -1 with the error recorded.
int stm_stream_set_layout(void *h, int layout, int tiles_x, int tiles_y, int order, int filter)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (!stm::layout_params_ok("stream_set_layout", layout, tiles_x, tiles_y, order, filter)) return -1;
    if (!not_submitted(f, "stream_set_layout")) return -1;
    if (layout == 0 && f->output.format == 1)
        return STM_REJECT("layout", "stream_set_layout: the stream's output format is 1 (NV12), which exists for quilts only: set format 0 first "
                          "(stm_stream_set_output)") ? 0 : -1;
    f->layout = layout == 0 ? stm::Layout{0, 1, 1, 0, 0} : stm::Layout{layout, tiles_x, tiles_y, order, filter};
    return 0;
}

// The output format of every frame of the stream (stm_set_output's formats and matrices; the default is format 0, BGR).  Format 1:
// each frame leaves as one contiguous NV12 surface, the Y plane of num_rows_out rows of num_cols_out bytes and the UV plane right
// behind it, num_rows_out * num_cols_out * 3 / 2 bytes in all -- that is what the download moves and a collect copies.  Kept and
// installed like the layout; the surface is screened against the stream's geometry by the first frame call.  Refused while the
// stream's layout is 0, and only before the first submit.  Returns 0, or -1 with the error recorded.
int stm_stream_set_output(void *h, int format, int matrix)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (!stm::output_params_ok("stream_set_output", format, matrix, 0, 0)) return -1;
    if (!not_submitted(f, "stream_set_output")) return -1;
    if (format == 1 && f->layout.layout == 0)
        return STM_REJECT("format", "stream_set_output: format 1 (NV12) exists for quilts only: set the stream's layout first "
                          "(stm_stream_set_layout)") ? 0 : -1;
    if (format == 1 && f->ov_max_rows > 0)
        return STM_REJECT("format", "stream_set_output: format 1 (NV12) together with the stream's overlay (stm_stream_set_overlay): compositing "
                          "on a chroma-subsampled surface is not defined, switch the overlay off first") ? 0 : -1;
    f->output = format == 0 ? stm::Output{0, 0, 0, 0} : stm::Output{1, matrix, 0, 0};
    f->out_bytes = format == 1 ? (size_t)f->Hout * f->Wout * 3 / 2 : f->out_sz;
    return 0;
}

// The overlay of the stream's frames (stm_hip.h): room for overlays of up to max_rows x max_cols pixels -- the stream's own host copy
// of the pixels in force and, per slot, a pinned and a device copy; (0, 0) = off.  Only before the first submit, and not together with
// output format 1.  Returns 0, or -1 with the error recorded and the stream unchanged.
int stm_stream_set_overlay(void *h, int max_rows, int max_cols)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    const bool off = max_rows == 0 && max_cols == 0;
    if (!off && (max_rows < 1 || max_rows > 65535 || max_cols < 1 || max_cols > 65535))
        return STM_REJECT("max_rows, max_cols", "stream_set_overlay: max_rows and max_cols must be in 1 .. 65535, or both 0 (off)") ? 0 : -1;
    if (!not_submitted(f, "stream_set_overlay")) return -1;
    if (!off && f->output.format == 1)
        return STM_REJECT("format", "stream_set_overlay: the stream's output format is 1 (NV12): compositing on a chroma-subsampled surface is not "
                          "defined, set format 0 first (stm_stream_set_output)") ? 0 : -1;
    int caller_dev = f->dev;
    STM_CHECK(hipGetDevice(&caller_dev));
    if (caller_dev != f->dev) STM_CHECK(hipSetDevice(f->dev));
    // the new buffers first, the old ones freed only once all exist: a failed allocation leaves the stream as it was
    const size_t bytes = (size_t)max_rows * max_cols * 4;
    u8 *pix = nullptr, *h_new[2] = {nullptr, nullptr}, *d_new[2] = {nullptr, nullptr};
    if (!off) {
        pix = (u8 *)malloc(bytes);
        if (!pix) stm::fail("stream_set_overlay: out of host memory", "malloc", __FILE__, __LINE__);
        for (int i = 0; i < 2 && !stm::failed(); ++i) {
            STM_CHECK(hipHostMalloc((void **)&h_new[i], bytes, hipHostMallocDefault));
            STM_CHECK(hipMalloc((void **)&d_new[i], bytes));
        }
    }
    if (stm::failed()) {
        free(pix);
        for (int i = 0; i < 2; ++i) {
            if (h_new[i]) (void)hipHostFree(h_new[i]);
            if (d_new[i]) (void)hipFree(d_new[i]);
        }
        if (caller_dev != f->dev) (void)hipSetDevice(caller_dev);
        return -1;
    }
    free(f->ov_pixels);
    f->ov_pixels = pix;
    for (int i = 0; i < 2; ++i) {
        Slot &s = f->slot[i];
        if (s.h_ov) STM_CHECK(hipHostFree(s.h_ov));
        if (s.d_ov) STM_CHECK(hipFree(s.d_ov));
        s.h_ov = h_new[i];
        s.d_ov = d_new[i];
        s.ov_gen = 0;
    }
    if (caller_dev != f->dev) STM_CHECK(hipSetDevice(caller_dev));
    f->ov_max_rows = max_rows;
    f->ov_max_cols = max_cols;
    f->ov = stm::Overlay{0, nullptr, 0, 0, 0, 0, 0.0f};
    f->ov_gen = 0;
    if (off) f->ov_auto.mode = 0; // the placement belongs to the overlay: set it again after the next stm_stream_set_overlay
    return 0;
}

// The automatic placement of the stream's overlay (stm_set_overlay_auto's rules; the default is mode 0).  Only before the first
// submit and after stm_stream_set_overlay.  Mode 1 allocates the stream's state -- 16 bytes at a fixed address, zeroed here, never by
// a memset node of a graph --, the fit's scratch and the slots' records.  Returns 0, or -1 with the error recorded and the stream unchanged.
int stm_stream_set_overlay_auto(void *h, int mode, int near_permille, float margin, int pad, float limit_lo, float limit_hi, float rate_near,
                                float rate_far)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (mode != 0 && mode != 1) return STM_REJECT("mode", "stream_set_overlay_auto: mode = %d, must be 0 (off) or 1 (on)", mode) ? 0 : -1;
    if (mode == 1 && (!stm::overlay_auto_params_ok("stream_set_overlay_auto", near_permille, margin, pad, limit_lo, limit_hi, rate_near, rate_far) ||
                      !stm::overlay_fit_size_ok("stream_set_overlay_auto", f->H, f->W)))
        return -1;
    if (!not_submitted(f, "stream_set_overlay_auto")) return -1;
    if (mode == 1 && f->ov_max_rows == 0)
        return STM_REJECT("stream", "stream_set_overlay_auto: the stream has no overlay (stm_stream_set_overlay comes first)") ? 0 : -1;
    if (mode == 1 && !f->d_ov_state) {
        int caller_dev = f->dev;
        STM_CHECK(hipGetDevice(&caller_dev));
        if (caller_dev != f->dev) STM_CHECK(hipSetDevice(f->dev));
        STM_CHECK(hipMalloc((void **)&f->d_ov_state, 16));
        STM_CHECK(hipMemset(f->d_ov_state, 0, 16)); // valid = 0: the first fit has no history
        STM_CHECK(hipMalloc((void **)&f->d_ov_ws, stm::OVERLAY_FIT_WS_WORDS * 4));
        for (Slot &s : f->slot) {
            STM_CHECK(hipMalloc((void **)&s.d_orec, 16));
            STM_CHECK(hipHostMalloc((void **)&s.h_orec, 16, hipHostMallocDefault));
            if (s.h_orec) memset(s.h_orec, 0, 16);
        }
        if (caller_dev != f->dev) STM_CHECK(hipSetDevice(caller_dev));
        if (stm::failed()) return -1;
    }
    f->ov_auto = mode == 0 ? stm::overlay_auto_default()
                           : stm::OverlayAuto{1, near_permille, margin, pad, limit_lo, limit_hi, rate_near, rate_far, f->d_ov_state};
    return 0;
}
// the overlay's state {valid, disparity, nearest, 0} as the most recently collected frame left it; with the placement off:
// {0, the disparity of stm_stream_overlay that frame was submitted under, 0, 0}
int stm_stream_overlay_depth(void *h, float out[4])
{
    FrameStream *f = (FrameStream *)h;
    if (f->collected == 0) return -1;
    const Slot &s = f->slot[(f->collected - 1) & 1];
    if (f->ov_auto.mode == 1) { for (int i = 0; i < 4; ++i) out[i] = s.h_orec[i]; }
    else { out[0] = 0.0f; out[1] = s.ov_disparity; out[2] = out[3] = 0.0f; }
    return 0;
}

// The overlay every later submit composites, until the next call (stm_hip.h): the pixels are copied into the stream's own memory, so the
// caller's are reusable on return; a slot uploads them when it next takes a frame.  NULL or a zero size = none.  Returns 0, or -1 with
// the error recorded and the overlay in force unchanged.
int stm_stream_overlay(void *h, const unsigned char *overlay, int ov_rows, int ov_cols, int x0, int y0, float disparity)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (f->ov_max_rows == 0)
        return STM_REJECT("stream", "stream_overlay: the stream has no overlay (stm_stream_set_overlay, before the first submit)") ? 0 : -1;
    if (!overlay || ov_rows == 0 || ov_cols == 0) {
        f->ov.mode = 0;
        return 0;
    }
    if (!stm::overlay_params_ok("stream_overlay", overlay, false, ov_rows, ov_cols, x0, y0, disparity)) return -1;
    if (ov_rows > f->ov_max_rows || ov_cols > f->ov_max_cols)
        return STM_REJECT("ov_rows, ov_cols", "stream_overlay: an overlay of %d x %d pixels, the stream holds at most %d x %d (stm_stream_set_overlay)",
                          ov_rows, ov_cols, f->ov_max_rows, f->ov_max_cols) ? 0 : -1;
    memcpy(f->ov_pixels, overlay, (size_t)ov_rows * ov_cols * 4);
    f->ov = stm::Overlay{1, nullptr, ov_rows, ov_cols, x0, y0, disparity};
    ++f->ov_gen;
    return 0;
}

// The depth budget every frame of the stream is rendered with (stm_set_depth's rules; the default is mode 0).  Kept and installed
// like the lens geometry.  Mode 2 allocates the stream's state and the slots' records.  Only before the first submit.
int stm_stream_set_depth(void *h, int mode, float gain, float conv)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (!stm::depth_params_ok("stream_set_depth", mode, gain, conv)) return -1;
    if (mode == 2 && !(f->depth.disp_lo < f->depth.disp_hi))
        return STM_REJECT("mode", "stream_set_depth: mode 2 (automatic) needs the budget of stm_stream_set_depth_auto first") ? 0 : -1;
    if (!not_submitted(f, "stream_set_depth")) return -1;
    if (mode == 2 && !f->d_depth_state) {
        STM_CHECK(hipMalloc((void **)&f->d_depth_state, 16));
        STM_CHECK(hipMemset(f->d_depth_state, 0, 16)); // valid = 0: the first frame starts the history
        for (Slot &s : f->slot) {
            STM_CHECK(hipMalloc((void **)&s.d_rec, 16));
            STM_CHECK(hipHostMalloc((void **)&s.h_rec, 16, hipHostMallocDefault));
        }
        if (stm::failed()) return -1;
    }
    f->depth.mode = mode;
    f->depth.gain = mode == 1 ? gain : 1.0f;
    f->depth.conv = mode == 1 ? conv : 0.0f;
    f->depth.d_state = f->d_depth_state;
    return 0;
}
// The view antialiasing of every frame of the stream (stm_set_antialias's rules; the default is mode 0).  Kept and installed like the
// depth budget, so the prefilter is part of the slots' captured graphs.  Only before the first submit.
int stm_stream_set_antialias(void *h, int mode, float strength, int max_radius, float gate)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (mode != 0 && mode != 1) return STM_REJECT("mode", "stream_set_antialias: mode = %d, must be 0 (off) or 1 (on)", mode) ? 0 : -1;
    if (mode == 1 && !stm::antialias_params_ok("stream_set_antialias", strength, max_radius, gate)) return -1;
    if (!not_submitted(f, "stream_set_antialias")) return -1;
    f->antialias = mode == 0 ? stm::Antialias{0, 0.0f, 0, 0.0f} : stm::Antialias{1, strength, max_radius, gate};
    return 0;
}
int stm_stream_set_depth_auto(void *h, float disp_lo, float disp_hi, float max_gain, int clip_permille, float rate)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (!stm::depth_auto_params_ok("stream_set_depth_auto", disp_lo, disp_hi, max_gain, clip_permille, rate)) return -1;
    if (!not_submitted(f, "stream_set_depth_auto")) return -1;
    f->depth.disp_lo = disp_lo; f->depth.disp_hi = disp_hi; f->depth.max_gain = max_gain; f->depth.clip_permille = clip_permille;
    f->depth.rate = rate;
    return 0;
}
// The vertical alignment every frame of the stream is conditioned with (stm_set_align's rules; the default is mode 0).  Kept and
// installed like the depth budget.  Mode 2 allocates the stream's state and the slots' records.  Only before the first submit.
int stm_stream_set_align(void *h, int mode, float a, float b, float c)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (!stm::align_params_ok("stream_set_align", mode, a, b, c)) return -1;
    if (!no_depth_input(f, "stream_set_align", "stream")) return -1; // ahead of the geometry rule: a depth frame has no second half
    if (!no_depth_video(f, "stream_set_align", "stream")) return -1;
    if (mode != 0 && !f->packing.on() && f->in_format == 0 && f->Wsbs < 2 * f->W)
        return STM_REJECT("num_cols_sbs", "stream_set_align: an alignment needs num_cols_sbs >= 2 * num_cols") ? 0 : -1;
    if (mode == 2 && !stm::align_size_ok("stream_set_align", f->H, f->W)) return -1;
    if (!not_submitted(f, "stream_set_align")) return -1;
    if (mode == 2 && !f->d_align_state) {
        STM_CHECK(hipMalloc((void **)&f->d_align_state, 16));
        STM_CHECK(hipMemset(f->d_align_state, 0, 16)); // valid = 0: the first frame starts the history
        for (Slot &s : f->slot) {
            STM_CHECK(hipMalloc((void **)&s.d_arec, 16));
            STM_CHECK(hipHostMalloc((void **)&s.h_arec, 16, hipHostMallocDefault));
        }
        if (stm::failed()) return -1;
    }
    f->align.mode = mode;
    f->align.a = mode == 1 ? a : 0.0f;
    f->align.b = mode == 1 ? b : 0.0f;
    f->align.c = mode == 1 ? c : 0.0f;
    f->align.d_state = f->d_align_state;
    return 0;
}
int stm_stream_set_align_auto(void *h, int radius, float rate)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (!stm::align_auto_params_ok("stream_set_align_auto", radius, rate)) return -1;
    if (!not_submitted(f, "stream_set_align_auto")) return -1;
    f->align.radius = radius;
    f->align.rate = rate;
    return 0;
}
// a, b and c applied to the most recently collected frame
int stm_stream_align(void *h, float out[3])
{
    FrameStream *f = (FrameStream *)h;
    if (f->collected == 0) return -1;
    const Slot &s = f->slot[(f->collected - 1) & 1];
    if (f->align.mode == 2) { out[0] = s.h_arec[1]; out[1] = s.h_arec[2]; out[2] = s.h_arec[3]; }
    else { out[0] = f->align.a; out[1] = f->align.b; out[2] = f->align.c; }
    return 0;
}
// The colour balance every frame of the stream is conditioned with (stm_set_balance's rules; the default is mode 0).  Kept and
// installed like the alignment.  Mode 2 allocates the stream's state and the slots' records.  Only before the first submit.
int stm_stream_set_balance(void *h, int mode, const unsigned char *lut768)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (!stm::balance_params_ok("stream_set_balance", mode, lut768)) return -1;
    if (!no_depth_input(f, "stream_set_balance", "stream")) return -1; // ahead of the geometry rule, as in stm_stream_set_align
    if (!no_depth_video(f, "stream_set_balance", "stream")) return -1;
    if (mode != 0 && !f->packing.on() && f->in_format == 0 && f->Wsbs < 2 * f->W)
        return STM_REJECT("num_cols_sbs", "stream_set_balance: a colour balance needs num_cols_sbs >= 2 * num_cols") ? 0 : -1;
    if (mode == 2 && !stm::balance_size_ok("stream_set_balance", f->H, f->W)) return -1;
    if (!not_submitted(f, "stream_set_balance")) return -1;
    const size_t bytes = stm::BALANCE_STATE_WORDS * 4;
    if (mode == 2 && !f->d_balance_state) {
        STM_CHECK(hipMalloc((void **)&f->d_balance_state, bytes));
        STM_CHECK(hipMemset(f->d_balance_state, 0, bytes)); // valid = 0: the first frame starts the history
        for (Slot &s : f->slot) {
            STM_CHECK(hipMalloc((void **)&s.d_brec, bytes));
            STM_CHECK(hipHostMalloc((void **)&s.h_brec, bytes, hipHostMallocDefault));
        }
        if (stm::failed()) return -1;
    }
    f->balance.mode = mode;
    for (int i = 0; i < 768; ++i) f->balance.lut[i] = mode == 1 ? lut768[i] : (unsigned char)i;
    f->balance.d_state = f->d_balance_state;
    return 0;
}
int stm_stream_set_balance_auto(void *h, int max_shift, float rate)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (!stm::balance_auto_params_ok("stream_set_balance_auto", max_shift, rate)) return -1;
    if (!not_submitted(f, "stream_set_balance_auto")) return -1;
    f->balance.max_shift = max_shift;
    f->balance.rate = rate;
    return 0;
}
// the tables applied to the most recently collected frame (mode 2: step 7 of stm_balance_apply on the slot's record of the state)
int stm_stream_balance(void *h, unsigned char out_lut[768])
{
    FrameStream *f = (FrameStream *)h;
    if (f->collected == 0) return -1;
    const Slot &s = f->slot[(f->collected - 1) & 1];
    for (int i = 0; i < 768; ++i) {
        if (f->balance.mode == 2) {
            const int v = (s.h_brec[1 + i] + 128) >> 8;
            out_lut[i] = (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
        } else {
            out_lut[i] = f->balance.lut[i];
        }
    }
    return 0;
}
// The shot-change detector of the stream's frames (stm_set_cut's rules; the default is mode 0).  Kept and installed like the balance.
// Mode 1 allocates the stream's state and the slots' records.  The reset pointers are the stream's own depth, alignment and balance
// states of mode 2, which the frame call resolves from the settings installed at submit: the setters may come in any order.  Only
// before the first submit.
int stm_stream_set_cut(void *h, int mode, int thresh_permille, int min_gap)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (mode != 0 && mode != 1) return STM_REJECT("mode", "stream_set_cut: mode = %d, must be 0 (off) or 1 (on)", mode) ? 0 : -1;
    if (mode == 1 && (!stm::cut_params_ok("stream_set_cut", thresh_permille, min_gap) || !stm::cut_size_ok("stream_set_cut", f->H, f->W))) return -1;
    if (!not_submitted(f, "stream_set_cut")) return -1;
    const size_t bytes = stm::CUT_STATE_WORDS * 4;
    if (mode == 1 && !f->d_cut_state) {
        STM_CHECK(hipMalloc((void **)&f->d_cut_state, bytes));
        STM_CHECK(hipMemset(f->d_cut_state, 0, bytes)); // valid = 0: the first frame is a cut
        for (Slot &s : f->slot) {
            STM_CHECK(hipMalloc((void **)&s.d_crec, 12));
            STM_CHECK(hipHostMalloc((void **)&s.h_crec, 12, hipHostMallocDefault));
        }
        if (stm::failed()) return -1;
    }
    f->cut.mode = mode;
    if (mode == 1) { f->cut.thresh_permille = thresh_permille; f->cut.min_gap = min_gap; }
    f->cut.d_state = mode == 1 ? f->d_cut_state : nullptr;
    return 0;
}
// The active picture area of the stream's frames (stm_set_active's and stm_set_active_auto's rules in one call; the default is mode
// 0).  Kept and installed like the cut detector.  The stream owns the state; the cut state mode 2 reads is the stream's own, which the
// frame call resolves from the settings installed at submit: the setters may come in any order.  Only before the first submit.
int stm_stream_set_active(void *h, int mode, const int rect[4], int fill, float fill_disp, int thresh_luma, int lit_permille, int max_bar_permille,
                          int hold)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (!stm::active_params_ok("stream_set_active", mode, rect, fill, fill_disp)) return -1;
    if (mode == 1 && !stm::active_rect_ok("stream_set_active", rect, f->H, f->W)) return -1;
    if (mode == 2 && (!stm::active_auto_params_ok("stream_set_active", thresh_luma, lit_permille, max_bar_permille, hold) ||
                      !stm::active_size_ok("stream_set_active", f->H, f->W)))
        return -1;
    if (!not_submitted(f, "stream_set_active")) return -1;
    const size_t bytes = stm::ACTIVE_STATE_WORDS * 4;
    if (mode != 0 && !f->d_active_state) {
        STM_CHECK(hipMalloc((void **)&f->d_active_state, bytes));
        for (Slot &s : f->slot) {
            STM_CHECK(hipMalloc((void **)&s.d_acrec, 20));
            STM_CHECK(hipHostMalloc((void **)&s.h_acrec, 20, hipHostMallocDefault));
        }
        if (stm::failed()) return -1;
    }
    if (mode != 0) { // mode 2: valid = 0, the first frame starts afresh; mode 1: the rectangle where the fits read it
        int st[stm::ACTIVE_STATE_WORDS] = {0};
        if (mode == 1) {
            st[0] = 1;
            for (int i = 0; i < 4; ++i) st[1 + i] = rect[i];
            st[6] = f->H; st[7] = f->W;
        }
        STM_CHECK(hipMemcpy(f->d_active_state, st, bytes, hipMemcpyHostToDevice));
        if (stm::failed()) return -1;
    }
    stm::Active a = f->active;
    a.mode = mode;
    for (int i = 0; i < 4; ++i) a.rect[i] = mode == 1 ? rect[i] : 0;
    a.fill = mode ? fill : 0;
    a.fill_disp = mode ? fill_disp : 0.0f;
    if (mode == 2) { a.thresh_luma = thresh_luma; a.lit_permille = lit_permille; a.max_bar_permille = max_bar_permille; a.hold = hold; }
    a.d_state = mode == 2 ? f->d_active_state : nullptr;
    f->active = a;
    return 0;
}
// {top, bottom, left, right, changed} of the most recently collected frame
int stm_stream_active(void *h, int out[5])
{
    FrameStream *f = (FrameStream *)h;
    if (f->collected == 0) return -1;
    const Slot &s = f->slot[(f->collected - 1) & 1];
    if (f->active.mode == 2) { for (int i = 0; i < 5; ++i) out[i] = s.h_acrec[i]; }
    else if (f->active.mode == 1) { for (int i = 0; i < 4; ++i) out[i] = f->active.rect[i]; out[4] = 0; }
    else { out[0] = 0; out[1] = f->H; out[2] = 0; out[3] = f->W; out[4] = 0; }
    return 0;
}
// {cut, score, since} of the most recently collected frame
int stm_stream_cut(void *h, int out[3])
{
    FrameStream *f = (FrameStream *)h;
    if (f->collected == 0) return -1;
    const Slot &s = f->slot[(f->collected - 1) & 1];
    if (f->cut.mode == 1) { out[0] = s.h_crec[0]; out[1] = s.h_crec[2]; out[2] = s.h_crec[1]; }
    else { out[0] = out[1] = out[2] = 0; }
    return 0;
}
// gain and conv applied to the most recently collected frame
int stm_stream_depth(void *h, float out[2])
{
    FrameStream *f = (FrameStream *)h;
    if (f->collected == 0) return -1;
    const Slot &s = f->slot[(f->collected - 1) & 1];
    if (f->depth.mode == 2) { out[0] = s.h_rec[1]; out[1] = s.h_rec[2]; }
    else { out[0] = f->depth.gain; out[1] = f->depth.conv; }
    return 0;
}

// What a frame's two disparity maps leave the stream as (stm_hip.h): format 0 = float32 (the default), 1 = not at all, 2 / 3 = u8 / u16
// planes of the maps selected by `which`, quantised between lo and hi.  The float maps are computed in every format.  Format 0 owns
// the slots' pinned float buffers, formats 2 and 3 a device and a pinned buffer per slot for the planes; whatever the new format does
// not download is freed, after everything it needs exists: a failed allocation leaves the stream as it was.  Only before the first
// submit.  Returns 0, or -1 with the error recorded and the stream unchanged.
int stm_stream_maps(void *h, int format, int which, float lo, float hi)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    if (format < 0 || format > 3)
        return STM_REJECT("format", "stream_maps: format = %d, must be 0 (float32 maps), 1 (no maps), 2 (u8 planes) or 3 (u16 planes)", format) ? 0 : -1;
    const bool planes = format >= 2;
    if (planes && (which < 0 || which > 2))
        return STM_REJECT("which", "stream_maps: which = %d, must be 0 (left), 1 (right) or 2 (both)", which) ? 0 : -1;
    if (planes && !(fabsf(lo) <= 4096.0f && fabsf(hi) <= 4096.0f)) // (NaN fails the comparison, inf the bound)
        return STM_REJECT("lo, hi", "stream_maps: lo and hi must be finite and in [-4096, 4096]") ? 0 : -1;
    if (planes && !(fabs((double)hi - (double)lo) >= 1.0 / 64.0))
        return STM_REJECT("lo, hi", "stream_maps: lo and hi must differ by at least 1/64") ? 0 : -1;
    if (!not_submitted(f, "stream_maps")) return -1;
    const int maxcode = format == 2 ? 255 : 65535, n = !planes ? 0 : which == 2 ? 2 : 1;
    const size_t plane_bytes = planes ? f->hw * (format == 2 ? 1 : 2) : 0;
    int caller_dev = f->dev;
    STM_CHECK(hipGetDevice(&caller_dev));
    if (caller_dev != f->dev) STM_CHECK(hipSetDevice(f->dev));
    float *h_dl[2] = {nullptr, nullptr}, *h_dr[2] = {nullptr, nullptr};
    u8 *d_pl[2] = {nullptr, nullptr}, *h_pl[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i) {
        if (format == 0 && !f->slot[i].h_dl) {
            STM_CHECK(hipHostMalloc((void **)&h_dl[i], f->hw * 4, hipHostMallocDefault));
            STM_CHECK(hipHostMalloc((void **)&h_dr[i], f->hw * 4, hipHostMallocDefault));
        }
        if (planes) {
            STM_CHECK(hipMalloc((void **)&d_pl[i], plane_bytes * n));
            STM_CHECK(hipHostMalloc((void **)&h_pl[i], plane_bytes * n, hipHostMallocDefault));
        }
    }
    if (stm::failed()) { // (error mode 1)
        for (int i = 0; i < 2; ++i) {
            if (h_dl[i]) (void)hipHostFree(h_dl[i]);
            if (h_dr[i]) (void)hipHostFree(h_dr[i]);
            if (d_pl[i]) (void)hipFree(d_pl[i]);
            if (h_pl[i]) (void)hipHostFree(h_pl[i]);
        }
        if (caller_dev != f->dev) (void)hipSetDevice(caller_dev);
        return -1;
    }
    for (int i = 0; i < 2; ++i) {
        Slot &s = f->slot[i];
        if (format == 0 && !s.h_dl) { s.h_dl = h_dl[i]; s.h_dr = h_dr[i]; }
        if (format != 0 && s.h_dl) {
            STM_CHECK(hipHostFree(s.h_dl)); STM_CHECK(hipHostFree(s.h_dr));
            s.h_dl = s.h_dr = nullptr;
        }
        if (s.d_pl) { STM_CHECK(hipFree(s.d_pl)); STM_CHECK(hipHostFree(s.h_pl)); }
        s.d_pl = d_pl[i];
        s.h_pl = h_pl[i];
    }
    if (caller_dev != f->dev) STM_CHECK(hipSetDevice(caller_dev));
    f->maps_format = format;
    f->maps_which = planes ? which : 2;
    f->maps_lo = planes ? lo : 0.0f;
    f->maps_k = planes ? (float)((double)maxcode / ((double)hi - (double)lo)) : 0.0f;
    f->plane_bytes = plane_bytes;
    f->planes = n;
    return 0;
}

// The stream's frames are an image and its depth plane (stm_depth_input.h has the definition): format -1 = off (the default), 0 = float32, 2 =
// u8, 3 = u16 codes between lo and hi; fill and gate of the hole filling.  A frame is then the image (num_rows * num_cols_sbs *
// elem_sz bytes) followed by the tight plane at the next multiple of 16 bytes, so each slot's pinned and device input buffers are
// allocated anew, after everything the new setting needs exists: pointers handed out by stm_stream_input_buffer before this call are
// void, and a failed allocation leaves the stream as it was.  Every frame is then computed by stm::depth_frame_device (no matcher).
// Not together with NV12 input, a packing, a match size, an alignment, a balance or stages beyond 3 | 0x800, in either order.  Only
// before the first submit.  Returns 0, or -1 with the error recorded and the stream unchanged.
int stm_stream_input_depth(void *h, int format, float lo, float hi, int fill, float gate)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    const char *fn = "stream_input_depth";
    if (format != -1 && format != 0 && format != 2 && format != 3)
        return STM_REJECT("format", "%s: format = %d, must be -1 (off), 0 (float32 plane), 2 (u8 plane) or 3 (u16 plane)", fn, format) ? 0 : -1;
    const bool on = format != -1;
    if (on && !(fabsf(lo) <= 4096.0f && fabsf(hi) <= 4096.0f)) // (NaN fails the comparison, inf the bound)
        return STM_REJECT("lo, hi", "%s: lo and hi must be finite and in [-4096, 4096]", fn) ? 0 : -1;
    if (on && !(fabs((double)hi - (double)lo) >= 1.0 / 64.0))
        return STM_REJECT("lo, hi", "%s: lo and hi must differ by at least 1/64", fn) ? 0 : -1;
    if (on && fill != 0 && fill != 1)
        return STM_REJECT("fill", "%s: fill = %d, must be 0 (constant extension) or 1 (continue the background)", fn, fill) ? 0 : -1;
    if (on && fill == 1 && !(gate >= 0.0f && gate <= 4096.0f)) // (NaN fails the comparison)
        return STM_REJECT("gate", "%s: gate must be finite and in [0, 4096]", fn) ? 0 : -1;
    if (on && f->W > 8192)
        return STM_REJECT("num_cols", "%s: the stream's num_cols = %d, must be <= 8192 (a row's keys live in LDS)", fn, f->W) ? 0 : -1;
    if (on && f->Wsbs < f->W)
        return STM_REJECT("num_cols_sbs", "%s: the stream's num_cols_sbs = %d, must be >= num_cols = %d", fn, f->Wsbs, f->W) ? 0 : -1;
    if (!not_submitted(f, fn)) return -1;
    if (on && !no_depth_video(f, fn, "stream")) return -1;
    if (on && f->in_format != 0)
        return STM_REJECT("input", "%s: the stream's input format is 1 (NV12, stm_stream_set_input): the image of a depth frame is BGR", fn) ? 0 : -1;
    if (on && f->packing.on())
        return STM_REJECT("packing", "%s: the stream has a packing (stm_stream_set_packing): a depth frame holds one image", fn) ? 0 : -1;
    if (on && f->match_h > 0)
        return STM_REJECT("match_size", "%s: the stream has a match size (stm_stream_set_match_size): nothing is matched", fn) ? 0 : -1;
    if (on && f->align.mode != 0)
        return STM_REJECT("align", "%s: the stream has an alignment (stm_stream_set_align): there is no second image to align", fn) ? 0 : -1;
    if (on && f->balance.mode != 0)
        return STM_REJECT("balance", "%s: the stream has a colour balance (stm_stream_set_balance): there is no second image to balance", fn) ? 0 : -1;
    if (on && f->rectify.mode != 0)
        return STM_REJECT("rectify", "%s: the stream has a rectification (stm_stream_rectify): an image-plus-depth frame is not rectified", fn) ? 0 : -1;
    if (on && (f->stages & ~0x800) != 3)
        return STM_REJECT("stages", "%s: the stream's stages are 0x%x (stm_stream_set_stages): a depth frame takes 3 or 3 | 0x800, nothing is "
                          "matched", fn, f->stages) ? 0 : -1;
    if (!on && f->din.format < 0) return 0; // off stays off: not one byte of the stream changes
    const size_t plane_off = (f->in_sz + 15) & ~(size_t)15;
    const size_t need = on ? plane_off + f->hw * (format == 0 ? 4 : format == 2 ? 1 : 2) : f->in_sz;
    int caller_dev = f->dev;
    STM_CHECK(hipGetDevice(&caller_dev));
    if (caller_dev != f->dev) STM_CHECK(hipSetDevice(f->dev));
    u8 *h_new[2] = {nullptr, nullptr}, *d_new[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i) {
        STM_CHECK(hipHostMalloc((void **)&h_new[i], need, hipHostMallocDefault));
        STM_CHECK(hipMalloc((void **)&d_new[i], need));
    }
    if (stm::failed()) { // (error mode 1; the hip calls take null pointers)
        for (int i = 0; i < 2; ++i) {
            if (h_new[i]) (void)hipHostFree(h_new[i]);
            if (d_new[i]) (void)hipFree(d_new[i]);
        }
        if (caller_dev != f->dev) (void)hipSetDevice(caller_dev);
        return -1;
    }
    for (int i = 0; i < 2; ++i) {
        Slot &s = f->slot[i];
        STM_CHECK(hipHostFree(s.h_in));
        STM_CHECK(hipFree(s.d_in));
        s.h_in = h_new[i];
        s.d_in = d_new[i];
    }
    if (caller_dev != f->dev) STM_CHECK(hipSetDevice(caller_dev));
    f->din = on ? stm::DepthInput{format, lo, hi, fill, fill == 1 ? gate : 0.0f} : stm::DepthInput{-1, 0.0f, 0.0f, 0, 0.0f};
    f->plane_off = on ? plane_off : 0;
    f->in_bytes = need;
    return 0;
}

// The stream's frames are packed 2D-plus-depth video frames (stm_depth_video.h has the definition): one BGR (format 0) or NV12 (1,
// converted by `matrix`) picture that holds the image as eye 0 and its depth picture as eye 1 of the packing (packing, swap, filter,
// gap: stm_stream_set_packing's settings and geometry rules on the stream's num_rows, num_cols_sbs and num_cols); range, dfilter,
// dgate, lo, hi decode the depth picture, fill and gate are stm_stream_input_depth's.  format -1 = off, the default.  A frame is then
// rows_f * num_cols_sbs * elem_sz bytes (NV12: * 3 / 2), so each slot's pinned and device input buffers are allocated anew, the old
// ones freed once all four new ones exist: pointers handed out by stm_stream_input_buffer before this call are void, and a failed
// allocation leaves the stream as it was.  Every frame is then computed by stm::depth_video_frame_device (no matcher).  Not together
// with stm_stream_input_depth, NV12 input or a packing of the stereo setters, a match size, an alignment, a balance, a rectification
// or stages beyond 3 | 0x800, in either order.  Only before the first submit.  Returns 0, or -1 with the error recorded and the
// stream unchanged.
int stm_stream_input_packed_depth(void *h, int format, int matrix, int packing, int swap, int filter, int gap, int range, int dfilter,
                                  int dgate, float lo, float hi, int fill, float gate)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    const char *fn = "stream_input_packed_depth";
    if (format != -1 && format != 0 && format != 1)
        return STM_REJECT("format", "%s: format = %d, must be -1 (off), 0 (BGR frame) or 1 (NV12 frame)", fn, format) ? 0 : -1;
    const bool on = format != -1;
    const stm::Packing pk = {packing, swap, filter, gap};
    if (on) {
        if (!stm::packing_params_ok(fn, pk)) return -1;
        if (range != 0 && range != 1)
            return STM_REJECT("range", "%s: range = %d, must be 0 (codes 0 .. 255) or 1 (limited-range video grey, 16 .. 235)", fn, range) ? 0 : -1;
        if (dfilter != 0 && dfilter != 1)
            return STM_REJECT("dfilter", "%s: dfilter = %d, must be 0 (replicate the depth sample) or 1 (linear inside a surface)", fn, dfilter) ? 0 : -1;
        if (dfilter != 0 && !(packing & 1))
            return STM_REJECT("dfilter", "%s: dfilter = %d with packing %d: a full-size depth picture is not expanded, dfilter must be 0", fn,
                              dfilter, packing) ? 0 : -1;
        if (dgate < 0 || dgate > 255) return STM_REJECT("dgate", "%s: dgate = %d, must be in 0 .. 255", fn, dgate) ? 0 : -1;
        if (!(fabsf(lo) <= 4096.0f && fabsf(hi) <= 4096.0f)) // (NaN fails the comparison, inf the bound)
            return STM_REJECT("lo, hi", "%s: lo and hi must be finite and in [-4096, 4096]", fn) ? 0 : -1;
        if (!(fabs((double)hi - (double)lo) >= 1.0 / 64.0)) return STM_REJECT("lo, hi", "%s: lo and hi must differ by at least 1/64", fn) ? 0 : -1;
        if (fill != 0 && fill != 1)
            return STM_REJECT("fill", "%s: fill = %d, must be 0 (constant extension) or 1 (continue the background)", fn, fill) ? 0 : -1;
        if (fill == 1 && !(gate >= 0.0f && gate <= 4096.0f)) // (NaN fails the comparison)
            return STM_REJECT("gate", "%s: gate must be finite and in [0, 4096]", fn) ? 0 : -1;
        if (f->W > 8192)
            return STM_REJECT("num_cols", "%s: the stream's num_cols = %d, must be <= 8192 (a row's keys live in LDS)", fn, f->W) ? 0 : -1;
        if (format == 1 && (f->Wsbs & 1)) // the UV plane follows the Y plane with the same pitch
            return STM_REJECT("num_cols_sbs", "%s: NV12 needs an even num_cols_sbs", fn) ? 0 : -1;
        if (!stm::packing_args_ok(fn, pk, f->H, f->Wsbs, f->W, "num_cols", format == 1, f->Wsbs, f->Wsbs, matrix)) return -1;
    }
    if (!not_submitted(f, fn)) return -1;
    if (on && f->din.format >= 0)
        return STM_REJECT("stream", "%s: the stream has depth input (stm_stream_input_depth): its frames are an image and a separate plane; "
                          "switch it off first", fn) ? 0 : -1;
    if (on && f->in_format != 0)
        return STM_REJECT("input", "%s: the stream's input format is 1 (NV12, stm_stream_set_input): the frame's format is this call's own "
                          "argument, set the stream's back to 0", fn) ? 0 : -1;
    if (on && f->packing.on())
        return STM_REJECT("packing", "%s: the stream has a packing (stm_stream_set_packing): the frame's packing is this call's own argument, "
                          "switch the stream's off", fn) ? 0 : -1;
    if (on && f->match_h > 0)
        return STM_REJECT("match_size", "%s: the stream has a match size (stm_stream_set_match_size): nothing is matched", fn) ? 0 : -1;
    if (on && f->align.mode != 0)
        return STM_REJECT("align", "%s: the stream has an alignment (stm_stream_set_align): there is no second image to align", fn) ? 0 : -1;
    if (on && f->balance.mode != 0)
        return STM_REJECT("balance", "%s: the stream has a colour balance (stm_stream_set_balance): there is no second image to balance", fn) ? 0 : -1;
    if (on && f->rectify.mode != 0)
        return STM_REJECT("rectify", "%s: the stream has a rectification (stm_stream_rectify): a 2D-plus-depth frame is not rectified", fn) ? 0 : -1;
    if (on && (f->stages & ~0x800) != 3)
        return STM_REJECT("stages", "%s: the stream's stages are 0x%x (stm_stream_set_stages): a 2D-plus-depth frame takes 3 or 3 | 0x800, nothing "
                          "is matched", fn, f->stages) ? 0 : -1;
    if (!on && f->dvid.format < 0) return 0; // off stays off: not one byte of the stream changes
    // (neither stereo setter is in force, so in_sz is the plain side-by-side frame the stream goes back to)
    const size_t frame_px = (size_t)pk.rows_f(f->H) * f->Wsbs;
    const size_t need = !on ? f->in_sz : format == 1 ? frame_px * 3 / 2 : frame_px * f->E;
    int caller_dev = f->dev;
    STM_CHECK(hipGetDevice(&caller_dev));
    if (caller_dev != f->dev) STM_CHECK(hipSetDevice(f->dev));
    u8 *h_new[2] = {nullptr, nullptr}, *d_new[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i) {
        STM_CHECK(hipHostMalloc((void **)&h_new[i], need, hipHostMallocDefault));
        STM_CHECK(hipMalloc((void **)&d_new[i], need));
    }
    if (stm::failed()) { // (error mode 1; the hip calls take null pointers)
        for (int i = 0; i < 2; ++i) {
            if (h_new[i]) (void)hipHostFree(h_new[i]);
            if (d_new[i]) (void)hipFree(d_new[i]);
        }
        if (caller_dev != f->dev) (void)hipSetDevice(caller_dev);
        return -1;
    }
    for (int i = 0; i < 2; ++i) {
        Slot &s = f->slot[i];
        STM_CHECK(hipHostFree(s.h_in));
        STM_CHECK(hipFree(s.d_in));
        s.h_in = h_new[i];
        s.d_in = d_new[i];
    }
    if (caller_dev != f->dev) STM_CHECK(hipSetDevice(caller_dev));
    f->dvid = on ? stm::DepthVideo{format, format == 1 ? matrix : 0, pk, range, dfilter, dgate, lo, hi, fill, fill == 1 ? gate : 0.0f}
                 : stm::DepthVideo{-1, 0, {0, 0, 0, 0}, 0, 0, 0, 0.0f, 0.0f, 0, 0.0f};
    f->in_bytes = need;
    return 0;
}

// The rectification every frame of the stream starts with (stm_rectify.h has the definition): mode 0 = off (the default), 1 = the
// left eye's record, then the right eye's, copied into the stream and installed around its frame calls like the alignment; the
// kernel takes them by value, so nothing is allocated.  Not together with depth input, in either order.  Only before the first
// submit.  Returns 0, or -1 with the error recorded and the stream unchanged.
int stm_stream_rectify(void *h, int mode, const float *rec36, int border)
{
    FrameStream *f = (FrameStream *)h;
    stm::clear_failed();
    const char *fn = "stream_rectify";
    if (mode != 0 && mode != 1) return STM_REJECT("mode", "%s: mode = %d, must be 0 (off) or 1 (both eyes through their records)", fn, mode) ? 0 : -1;
    if (mode == 1) {
        if (!stm::ptrs_ok(fn, {{"rec36", rec36}})) return -1;
        if (!stm::rectify_params_ok(fn, rec36, border) || !stm::rectify_params_ok(fn, rec36 + 18, border)) return -1;
    }
    if (mode != 0 && !no_depth_input(f, fn, "stream")) return -1; // ahead of the geometry rule, as in stm_stream_set_align
    if (mode != 0 && !no_depth_video(f, fn, "stream")) return -1;
    if (mode != 0 && !f->packing.on() && f->in_format == 0 && f->Wsbs < 2 * f->W)
        return STM_REJECT("num_cols_sbs", "%s: a rectification needs num_cols_sbs >= 2 * num_cols", fn) ? 0 : -1;
    if (!not_submitted(f, fn)) return -1;
    stm::Rectify r = {0, {{0.0f}, {0.0f}}, 0};
    if (mode == 1) {
        r.mode = 1;
        r.border = border;
        memcpy(r.rec, rec36, sizeof r.rec);
    }
    f->rectify = r;
    return 0;
}
int stm_stream_get_rectify(void *h, int *mode, float *rec36, int *border)
{
    const FrameStream *f = (const FrameStream *)h;
    if (!f) return -1;
    if (mode) *mode = f->rectify.mode;
    if (rec36 && f->rectify.mode) memcpy(rec36, f->rectify.rec, sizeof f->rectify.rec);
    if (border && f->rectify.mode) *border = f->rectify.border;
    return 0;
}

// Stage frame `submitted`; at most two frames may be in flight (collect the older one first).
// Returns the frame's index, or -1 when both slots are still uncollected.
long stm_stream_submit(void *h, const unsigned char *img_sbs)
{
    FrameStream *f = (FrameStream *)h;
    Slot &s = f->slot[f->submitted & 1];
    if (s.busy) return -1;
    stm::clear_failed();
    int caller_dev = f->dev;
    STM_CHECK(hipGetDevice(&caller_dev));
    if (caller_dev != f->dev) STM_CHECK(hipSetDevice(f->dev));
    // the caller's buffer is free again when this returns (as with adcensus_stm); a frame that was written straight into the
    // slot's pinned buffer (stm_stream_input_buffer) needs no copy
    if (img_sbs && img_sbs != s.h_in) memcpy(s.h_in, img_sbs, f->in_bytes);
    // temporal stabilisation: frame k reads the input and the maps of frame k - 1, which live in the other slot.  So the upload
    // into this slot's d_in waits until the other slot's frame (which may still be reading this d_in as ITS history) is done,
    // and this frame's compute waits for the other slot's outputs.  The two frames in flight then no longer overlap on the GPU;
    // upload and download still do.  The other slot's ev_done was recorded by the previous submit.
    Slot &other = f->slot[(f->submitted & 1) ^ 1];
    const bool temporal = (f->stages & 0x2000) != 0, history = temporal && f->submitted > 0;
    // depth mode 2: frame k's fit reads the state frame k - 1 wrote, so its compute waits for the other slot's frame as well
    const bool depth_auto = f->depth.mode == 2;
    const bool align_auto = f->align.mode == 2; // likewise the alignment's state
    const bool balance_auto = f->balance.mode == 2; // ... and the colour balance's
    const bool cut_on = f->cut.mode == 1;           // ... and the shot-change detector's
    const bool ov_auto = f->ov_auto.mode == 1;      // ... and the overlay placement's, which also reads the depth and the cut state
    const bool active_auto = f->active.mode == 2;   // ... and the active area's, which also reads the cut state
    // In NV12 mode the history is the other slot's converted split images (d_img_l / d_img_r), which no upload touches, and this
    // slot's d_in was last read by this slot's own previous frame, collected before the slot was handed out again: the upload
    // waits for nothing.  This frame's compute still waits for the other slot's frame: it reads that frame's images and maps, and
    // writes the images that frame reads as ITS history.
    if (history && f->in_format == 0) STM_CHECK(hipStreamWaitEvent(f->s_in, other.ev_done, 0));
    STM_CHECK(hipMemcpyAsync(s.d_in, s.h_in, f->in_bytes, hipMemcpyHostToDevice, f->s_in));
    // the overlay in force (stm_stream_overlay): a slot whose device copy holds another call's pixels uploads them ahead of the
    // frame.  The slot's previous frame, the last reader of both copies, was collected before the slot was handed out again.
    const stm::Overlay ov = f->ov;
    if (ov.mode == 1 && s.ov_gen != f->ov_gen) {
        const size_t ov_bytes = (size_t)ov.ov_rows * ov.ov_cols * 4;
        memcpy(s.h_ov, f->ov_pixels, ov_bytes);
        STM_CHECK(hipMemcpyAsync(s.d_ov, s.h_ov, ov_bytes, hipMemcpyHostToDevice, f->s_in));
        s.ov_gen = f->ov_gen;
    }
    STM_CHECK(hipEventRecord(s.ev_in, f->s_in));
    STM_CHECK(hipStreamWaitEvent(s.s_compute, s.ev_in, 0));
    if (history || ((depth_auto || align_auto || balance_auto || cut_on || ov_auto || active_auto) && f->submitted > 0)) STM_CHECK(hipStreamWaitEvent(s.s_compute, other.ev_done, 0));
    void *prev = stm_get_stream();
    LensScope lens_scope(f->lens);
    LayoutScope layout_scope(f->layout);
    OutputScope output_scope(f->output);
    DepthScope depth_scope(f->depth);
    AntialiasScope antialias_scope(f->antialias);
    AlignScope align_scope(f->align);
    RectifyScope rectify_scope(f->rectify);
    BalanceScope balance_scope(f->balance);
    CutScope cut_scope(f->cut);
    ActiveScope active_scope(f->active);
    PackingScope packing_scope(f->packing);
    OverlayOffScope overlay_scope;
    AggTapOffScope agg_tap_scope;
    stm_set_stream(s.s_compute);
    stm::ws_private_bind(s.ws);
    auto frame = [&]() {
        stm::ApiNest nest; // a failed upload above must survive the nested call's argument screen
        if (f->dvid.format >= 0) { // one packed frame, the image in one half and its depth picture in the other: likewise, from that frame
            stm::depth_video_frame_device(s.d_in, f->dvid, s.d_dl, s.d_dr, s.d_out, f->H, f->Wsbs, f->W, f->Hout, f->Wout, f->E, f->N, f->angle,
                                          f->stages);
            return;
        }
        if (f->din.format >= 0) { // an image and its depth plane: the second eye, then the stereo frame's own tail (no matcher)
            stm::depth_frame_device(s.d_in, s.d_in + f->plane_off, f->din, s.d_dl, s.d_dr, s.d_out, f->H, f->Wsbs, f->W, f->Hout, f->Wout, f->E,
                                    f->N, f->angle, f->stages);
            return;
        }
        if (f->match_h > 0) { // the reduced-resolution frame, picked as below
            if (f->in_format == 1) {
                stm_d_adcensus_stm_2nv12(s.d_in, f->Wsbs, s.d_in + (size_t)f->rows_f * f->Wsbs, f->Wsbs, f->in_matrix, s.d_dl, s.d_dr, s.d_out,
                                         f->H, f->Wsbs, f->W, f->Hout, f->Wout, f->match_h, f->match_w, f->E, f->match_scale, f->N, f->angle,
                                         f->D, f->zd, f->ad, f->ce, f->ucd, f->lcd, f->usd, f->lsd, f->thresh_s, f->thresh_h, f->stages,
                                         history ? other.d_img_l : nullptr, history ? other.d_img_r : nullptr, history ? other.d_dl : nullptr,
                                         history ? other.d_dr : nullptr, f->t_alpha, f->t_color, f->t_disp, s.d_img_l, s.d_img_r);
            } else if (temporal) {
                stm_d_adcensus_stm_2t(s.d_in, s.d_dl, s.d_dr, s.d_out, f->H, f->Wsbs, f->W, f->Hout, f->Wout, f->match_h, f->match_w, f->E,
                                      f->match_scale, f->N, f->angle, f->D, f->zd, f->ad, f->ce, f->ucd, f->lcd, f->usd, f->lsd, f->thresh_s,
                                      f->thresh_h, f->stages, history ? other.d_in : nullptr, history ? other.d_dl : nullptr,
                                      history ? other.d_dr : nullptr, f->t_alpha, f->t_color, f->t_disp);
            } else {
                stm_d_adcensus_stm_2s(s.d_in, s.d_dl, s.d_dr, s.d_out, f->H, f->Wsbs, f->W, f->Hout, f->Wout, f->match_h, f->match_w, f->E,
                                      f->match_scale, f->N, f->angle, f->D, f->zd, f->ad, f->ce, f->ucd, f->lcd, f->usd, f->lsd, f->thresh_s,
                                      f->thresh_h, f->stages);
            }
            return;
        }
        if (f->in_format == 1) { // NV12: the slot's images receive the conversion; with 0x2000 the other slot's images and maps are the history
            stm_d_adcensus_stm_nv12(s.d_in, f->Wsbs, s.d_in + (size_t)f->rows_f * f->Wsbs, f->Wsbs, f->in_matrix, s.d_dl, s.d_dr, s.d_out, f->H,
                                    f->Wsbs, f->W, f->Hout, f->Wout, f->E, f->N, f->angle, f->D, f->zd, f->ad, f->ce, f->ucd, f->lcd,
                                    f->usd, f->lsd, f->thresh_s, f->thresh_h, f->stages, history ? other.d_img_l : nullptr,
                                    history ? other.d_img_r : nullptr, history ? other.d_dl : nullptr, history ? other.d_dr : nullptr,
                                    f->t_alpha, f->t_color, f->t_disp, s.d_img_l, s.d_img_r);
            return;
        }
        if (temporal) { // the history pointers are fixed per slot: a captured frame (never the stream's first) replays them
            stm_d_adcensus_stm_t(s.d_in, s.d_dl, s.d_dr, s.d_out, f->H, f->Wsbs, f->W, f->Hout, f->Wout, f->E, f->N, f->angle, f->D,
                                 f->zd, f->ad, f->ce, f->ucd, f->lcd, f->usd, f->lsd, f->thresh_s, f->thresh_h, f->stages,
                                 history ? other.d_in : nullptr, history ? other.d_dl : nullptr, history ? other.d_dr : nullptr,
                                 f->t_alpha, f->t_color, f->t_disp);
            return;
        }
        stm_d_adcensus_stm(s.d_in, s.d_dl, s.d_dr, s.d_out, f->H, f->Wsbs, f->W, f->Hout, f->Wout, f->E, f->N, f->angle, f->D,
                           f->zd, f->ad, f->ce, f->ucd, f->lcd, f->usd, f->lsd, f->thresh_s, f->thresh_h, f->stages);
    };
    // stm_stream_maps, formats 2 and 3: the planes are quantised right behind the frame, from the float maps it left in d_dl / d_dr
    // (which stay what 0x2000's history and the overlay fit read).  The launch's arguments are the slot's own buffers and the
    // stream's settings, fixed from the first submit on, so it is part of what the slot captures and replays with the graph
    auto pipeline = [&]() {
        frame();
        if (f->planes > 0) {
            const float *src[2] = {f->maps_which == 1 ? s.d_dr : s.d_dl, s.d_dr};
            void *dst[2] = {s.d_pl, s.d_pl + f->plane_bytes};
            stm::launch_disp_plane(f->planes, src, dst, f->hw, f->maps_format == 2 ? 1 : 2, f->maps_lo, f->maps_k);
        }
    };
    void *wb = nullptr;
    size_t wc = 0;
    stm::ws_identity(&wb, &wc);
    if (s.gexec && (wb != s.g_ws_base || wc != s.g_ws_cap)) { // cannot happen with a private workspace; never replay stale addresses
        STM_CHECK(hipGraphExecDestroy(s.gexec));
        s.gexec = nullptr;
    }
    if (s.gexec) {
        STM_CHECK(hipGraphLaunch(s.gexec, s.s_compute));
    } else if (f->use_graph && s.eager_runs >= 1 && !stm::prof_enabled()) {
        // the slot's first frame ran eagerly (it sized the workspace, built the lookup tables, raised the LDS limits), so
        // nothing in here allocates or synchronises: capture this frame's launches, then run the capture
        hipGraph_t graph = nullptr;
        STM_CHECK(hipStreamBeginCapture(s.s_compute, hipStreamCaptureModeThreadLocal));
        pipeline();
        const bool capture_failed = stm::failed(); // error mode 1: something inside the capture recorded an error
        STM_CHECK(hipStreamEndCapture(s.s_compute, &graph)); // always leave capture mode
        if (capture_failed || !graph) {
            if (graph) STM_CHECK(hipGraphDestroy(graph));
            f->use_graph = false; // stay eager from now on
            stm::ws_private_bind(nullptr);
            stm_set_stream(prev);
            if (caller_dev != f->dev) STM_CHECK(hipSetDevice(caller_dev));
            return -1;
        }
        STM_CHECK(hipGraphInstantiate(&s.gexec, graph, nullptr, nullptr, 0));
        STM_CHECK(hipGraphDestroy(graph));
        stm::ws_identity(&s.g_ws_base, &s.g_ws_cap);
        STM_CHECK(hipGraphLaunch(s.gexec, s.s_compute));
    } else {
        pipeline();
        ++s.eager_runs;
    }
    // the overlay, composited on the slot's finished frame: a launch of its own behind the graph (or the eager pipeline) on the slot's
    // compute stream, so its arguments change from frame to frame without touching the capture.  With the automatic placement the fit's
    // launches go in front of it in the same way: they read this frame's maps and the depth and cut states its pipeline left, and the
    // overlay's state the previous frame left (the wait on the other slot's ev_done above).  A new overlay has no continuity to keep
    s.ov_disparity = ov.mode == 1 ? ov.disparity : 0.0f;
    if (ov.mode == 1 && ov_auto) {
        stm::frame_overlay_auto(s.d_out, stm::Overlay{1, s.d_ov, ov.ov_rows, ov.ov_cols, ov.x0, ov.y0, ov.disparity}, f->ov_auto, f->d_ov_state,
                                f->d_ov_ws, f->ov_gen != f->ov_fit_gen, false, s.d_dl, s.d_dr, f->H, f->W, f->depth, f->depth.d_state,
                                cut_on ? f->d_cut_state : nullptr, f->lens, f->layout, f->N, f->angle, f->Hout, f->Wout, f->E,
                                f->active.mode ? f->d_active_state + 1 : nullptr);
        f->ov_fit_gen = f->ov_gen;
    } else if (ov.mode == 1) {
        stm::frame_overlay(s.d_out, stm::Overlay{1, s.d_ov, ov.ov_rows, ov.ov_cols, ov.x0, ov.y0, ov.disparity}, f->lens, f->layout, f->N,
                           f->angle, f->Hout, f->Wout, f->E);
    }
    stm::ws_private_bind(nullptr);
    stm_set_stream(prev);
    // the state as this frame left it, before ev_done lets the next frame's fit update it
    if (depth_auto) STM_CHECK(hipMemcpyAsync(s.d_rec, f->d_depth_state, 16, hipMemcpyDeviceToDevice, s.s_compute));
    if (align_auto) STM_CHECK(hipMemcpyAsync(s.d_arec, f->d_align_state, 16, hipMemcpyDeviceToDevice, s.s_compute));
    if (balance_auto)
        STM_CHECK(hipMemcpyAsync(s.d_brec, f->d_balance_state, stm::BALANCE_STATE_WORDS * 4, hipMemcpyDeviceToDevice, s.s_compute));
    if (cut_on) STM_CHECK(hipMemcpyAsync(s.d_crec, f->d_cut_state + 1, 12, hipMemcpyDeviceToDevice, s.s_compute));
    if (ov_auto) STM_CHECK(hipMemcpyAsync(s.d_orec, f->d_ov_state, 16, hipMemcpyDeviceToDevice, s.s_compute));
    if (active_auto) STM_CHECK(hipMemcpyAsync(s.d_acrec, f->d_active_state + 1, 20, hipMemcpyDeviceToDevice, s.s_compute));
    STM_CHECK(hipEventRecord(s.ev_done, s.s_compute));
    STM_CHECK(hipStreamWaitEvent(f->s_out, s.ev_done, 0));
    if (f->maps_format == 0) {
        STM_CHECK(hipMemcpyAsync(s.h_dl, s.d_dl, f->hw * 4, hipMemcpyDeviceToHost, f->s_out));
        STM_CHECK(hipMemcpyAsync(s.h_dr, s.d_dr, f->hw * 4, hipMemcpyDeviceToHost, f->s_out));
    } else if (f->planes > 0) { // the planes in place of the float maps; format 1 downloads the frame alone
        STM_CHECK(hipMemcpyAsync(s.h_pl, s.d_pl, f->plane_bytes * f->planes, hipMemcpyDeviceToHost, f->s_out));
    }
    STM_CHECK(hipMemcpyAsync(s.h_out, s.d_out, f->out_bytes, hipMemcpyDeviceToHost, f->s_out));
    if (depth_auto) STM_CHECK(hipMemcpyAsync(s.h_rec, s.d_rec, 16, hipMemcpyDeviceToHost, f->s_out));
    if (align_auto) STM_CHECK(hipMemcpyAsync(s.h_arec, s.d_arec, 16, hipMemcpyDeviceToHost, f->s_out));
    if (balance_auto) STM_CHECK(hipMemcpyAsync(s.h_brec, s.d_brec, stm::BALANCE_STATE_WORDS * 4, hipMemcpyDeviceToHost, f->s_out));
    if (cut_on) STM_CHECK(hipMemcpyAsync(s.h_crec, s.d_crec, 12, hipMemcpyDeviceToHost, f->s_out));
    if (ov_auto) STM_CHECK(hipMemcpyAsync(s.h_orec, s.d_orec, 16, hipMemcpyDeviceToHost, f->s_out));
    if (active_auto) STM_CHECK(hipMemcpyAsync(s.h_acrec, s.d_acrec, 20, hipMemcpyDeviceToHost, f->s_out));
    STM_CHECK(hipEventRecord(s.ev_out, f->s_out));
    if (caller_dev != f->dev) STM_CHECK(hipSetDevice(caller_dev));
    if (stm::failed()) return -1; // error mode 1: the frame was not (completely) enqueued
    s.busy = true;
    return f->submitted++;
}

// Blocks until the oldest uncollected frame is complete and copies its results out (any pointer may be NULL).
// Returns that frame's index, or -1 when nothing is pending.
long stm_stream_collect(void *h, float *disp_l, float *disp_r, unsigned char *interlaced)
{
    FrameStream *f = (FrameStream *)h;
    if (f->collected >= f->submitted) return -1;
    if (!float_maps_ok(f, "stream_collect", disp_l, disp_r)) return -1;
    Slot &s = f->slot[f->collected & 1];
    STM_CHECK(hipEventSynchronize(s.ev_out));
    if (disp_l) memcpy(disp_l, s.h_dl, f->hw * 4);
    if (disp_r) memcpy(disp_r, s.h_dr, f->hw * 4);
    if (interlaced) memcpy(interlaced, s.h_out, f->out_bytes);
    s.busy = false;
    return f->collected++;
}

// Zero-copy variants: at 1080p the two host-side copies (12 MB in, 23 MB out) take longer than the frame does on the GPU.
// The pinned input buffer of the slot the NEXT submit will use: decode / write the frame into it, then call
// stm_stream_submit(stream, that pointer) (or NULL).  NULL while that slot is still uncollected.
unsigned char *stm_stream_input_buffer(void *h)
{
    FrameStream *f = (FrameStream *)h;
    Slot &s = f->slot[f->submitted & 1];
    return s.busy ? nullptr : s.h_in;
}

// Waits for the oldest uncollected frame and hands out pointers to its pinned result buffers instead of copying them; the
// pointers stay valid until the frame after the next one is submitted (its slot is reused then).  Returns the index or -1.
long stm_stream_collect_view(void *h, const float **disp_l, const float **disp_r, const unsigned char **interlaced)
{
    FrameStream *f = (FrameStream *)h;
    if (f->collected >= f->submitted) return -1;
    if (!float_maps_ok(f, "stream_collect_view", disp_l, disp_r)) return -1;
    Slot &s = f->slot[f->collected & 1];
    STM_CHECK(hipEventSynchronize(s.ev_out));
    if (disp_l) *disp_l = s.h_dl;
    if (disp_r) *disp_r = s.h_dr;
    if (interlaced) *interlaced = s.h_out;
    s.busy = false;
    return f->collected++;
}

// The collects of a stream whose maps leave as planes, or not at all (stm_stream_maps, formats 1 to 3; stm_hip.h): as
// stm_stream_collect and stm_stream_collect_view, with the planes in place of the float maps.  A plane the stream does not produce
// has nothing to copy -- a destination for it is refused, and nothing is consumed -- and its view is NULL.
long stm_stream_collect_maps(void *h, void *plane_l, void *plane_r, unsigned char *interlaced)
{
    FrameStream *f = (FrameStream *)h;
    if (f->collected >= f->submitted) return -1;
    if (!planes_ok(f, "stream_collect_maps", plane_l, plane_r)) return -1;
    Slot &s = f->slot[f->collected & 1];
    STM_CHECK(hipEventSynchronize(s.ev_out));
    if (plane_l) memcpy(plane_l, s.h_pl, f->plane_bytes);
    if (plane_r) memcpy(plane_r, s.h_pl + (f->planes == 2 ? f->plane_bytes : 0), f->plane_bytes);
    if (interlaced) memcpy(interlaced, s.h_out, f->out_bytes);
    s.busy = false;
    return f->collected++;
}

long stm_stream_collect_maps_view(void *h, const void **plane_l, const void **plane_r, const unsigned char **interlaced)
{
    FrameStream *f = (FrameStream *)h;
    if (f->collected >= f->submitted) return -1;
    if (!planes_ok(f, "stream_collect_maps_view", nullptr, nullptr)) return -1;
    Slot &s = f->slot[f->collected & 1];
    STM_CHECK(hipEventSynchronize(s.ev_out));
    const bool left = f->planes > 0 && f->maps_which != 1, right = f->planes > 0 && f->maps_which != 0;
    if (plane_l) *plane_l = left ? s.h_pl : nullptr;
    if (plane_r) *plane_r = right ? s.h_pl + (f->planes == 2 ? f->plane_bytes : 0) : nullptr;
    if (interlaced) *interlaced = s.h_out;
    s.busy = false;
    return f->collected++;
}

void stm_stream_destroy(void *h)
{
    FrameStream *f = (FrameStream *)h;
    if (!f) return;
    STM_CHECK(hipStreamSynchronize(f->s_in));
    for (Slot &s : f->slot) STM_CHECK(hipStreamSynchronize(s.s_compute));
    STM_CHECK(hipStreamSynchronize(f->s_out));
    for (Slot &s : f->slot) {
        STM_CHECK(hipHostFree(s.h_in)); STM_CHECK(hipHostFree(s.h_out));
        if (s.h_dl) { STM_CHECK(hipHostFree(s.h_dl)); STM_CHECK(hipHostFree(s.h_dr)); }
        if (s.d_pl) { STM_CHECK(hipFree(s.d_pl)); STM_CHECK(hipHostFree(s.h_pl)); }
        STM_CHECK(hipFree(s.d_in)); STM_CHECK(hipFree(s.d_out)); STM_CHECK(hipFree(s.d_dl)); STM_CHECK(hipFree(s.d_dr));
        STM_CHECK(hipEventDestroy(s.ev_in)); STM_CHECK(hipEventDestroy(s.ev_done)); STM_CHECK(hipEventDestroy(s.ev_out));
        if (s.gexec) STM_CHECK(hipGraphExecDestroy(s.gexec));
        if (s.d_img_l) STM_CHECK(hipFree(s.d_img_l));
        if (s.d_img_r) STM_CHECK(hipFree(s.d_img_r));
        if (s.d_rec) STM_CHECK(hipFree(s.d_rec));
        if (s.h_rec) STM_CHECK(hipHostFree(s.h_rec));
        if (s.d_arec) STM_CHECK(hipFree(s.d_arec));
        if (s.h_arec) STM_CHECK(hipHostFree(s.h_arec));
        if (s.d_brec) STM_CHECK(hipFree(s.d_brec));
        if (s.h_brec) STM_CHECK(hipHostFree(s.h_brec));
        if (s.d_crec) STM_CHECK(hipFree(s.d_crec));
        if (s.d_acrec) STM_CHECK(hipFree(s.d_acrec));
        if (s.h_acrec) STM_CHECK(hipHostFree(s.h_acrec));
        if (s.h_crec) STM_CHECK(hipHostFree(s.h_crec));
        if (s.h_ov) STM_CHECK(hipHostFree(s.h_ov));
        if (s.d_ov) STM_CHECK(hipFree(s.d_ov));
        if (s.d_orec) STM_CHECK(hipFree(s.d_orec));
        if (s.h_orec) STM_CHECK(hipHostFree(s.h_orec));
    }
    free(f->ov_pixels);
    if (f->d_ov_state) STM_CHECK(hipFree(f->d_ov_state));
    if (f->d_ov_ws) STM_CHECK(hipFree(f->d_ov_ws));
    if (f->d_depth_state) STM_CHECK(hipFree(f->d_depth_state));
    if (f->d_align_state) STM_CHECK(hipFree(f->d_align_state));
    if (f->d_balance_state) STM_CHECK(hipFree(f->d_balance_state));
    if (f->d_cut_state) STM_CHECK(hipFree(f->d_cut_state));
    if (f->d_active_state) STM_CHECK(hipFree(f->d_active_state));
    stm::ws_private_destroy(f->slot[0].ws);
    STM_CHECK(hipStreamDestroy(f->slot[0].s_compute));
    if (f->overlap) {
        stm::ws_private_destroy(f->slot[1].ws);
        STM_CHECK(hipStreamDestroy(f->slot[1].s_compute));
    }
    STM_CHECK(hipStreamDestroy(f->s_in)); STM_CHECK(hipStreamDestroy(f->s_out));
    delete f;
}

} // extern "C"
