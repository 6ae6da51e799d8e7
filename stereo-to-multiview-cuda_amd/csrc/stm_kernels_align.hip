// stm_kernels_align.hip -- vertical alignment of the stereo pair (stm_set_align, stm_align_rows, stm_align_fit; include/stm_hip.h has
// the definition line by line).  An addition, the reference has nothing like it: it takes rectified studio masters.  Four kernels:
//   stm_k_align_profiles  per eye, column band and row the sum of grey over the band, read straight from the caller's input (BGR or
//                         NV12, any packing): one wave per segment, a wave reduction, one store;
//   stm_k_align_sad       the vertical gradients of the profiles and their sums of absolute differences over the search range: one
//                         workgroup per (band, row block), the offsets spread over lanes;
//   stm_k_align_fit       one wave: per block the minimum, its parabola and weight; on one lane the weighted plane fit in f64 and the
//                         update of the four-float state;
//   stm_k_align_frame     the field applied: the aligned, unpacked, converted pair written as one side-by-side BGR frame, which the
//                         plain frame path then takes.  With one image it is the stage stm_d_align_rows.
// No atomics and integer sums only before the fit, so nothing depends on the order anything ran in.  Nothing is read back: the state
// stays in device memory (as the depth budget's, stm_kernels_depth.hip), so a frame stream's captured graphs replay the measurement.
#include "stm_common.h"
#include "stm_fetch.h"

namespace stm {

namespace {

constexpr int AL_KB = 8, AL_KR = 4, AL_RMAX = 32;

// grey = (u8)(b*c + g*c + r*c) as stm_kernels_cost.hip's grey_of (d_mux_common.cu:16-20)
__device__ __forceinline__ uint32_t al_grey_of(uint32_t px)
{
    const float c = 0.33333334f;
    float b = (float)(px & 0xff) * c;
    float g = (float)((px >> 8) & 0xff) * c;
    float r = (float)((px >> 16) & 0xff) * c;
    float s = b + g;
    s = s + r;
    return (uint32_t)s;
}

// ---------------------------------------------------------------- step 1: the profiles
// prof[(e * KB + j) * H + y] = the sum of grey over band j of row y of eye e.  Segment = (eye, row, band), band fastest: the four waves
// of a block read neighbouring stretches of one row.
template <int FMT, int AXIS, int FILT>
__global__ __launch_bounds__(256) void stm_k_align_profiles(uint32_t *__restrict__ prof, AlignSrc s, int H, int W)
{
    const int lane = threadIdx.x & 63;
    const long long seg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= 2ll * H * AL_KB) return; // (the whole wave)
    const int band = (int)(seg % AL_KB);
    const long long t = seg / AL_KB;
    const int y = (int)(t % H), eye = (int)(t / H);
    const int x0 = (int)((long long)band * W / AL_KB), x1 = (int)((long long)(band + 1) * W / AL_KB);
    uint32_t sum = 0;
    for (int x = x0 + lane; x < x1; x += 64) sum += al_grey_of(al_unpacked_px<FMT, AXIS, FILT>(s, eye, y, x));
#pragma unroll
    for (int d = 32; d; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d);
    if (lane == 0) prof[((size_t)eye * AL_KB + band) * H + y] = sum;
}

// ---------------------------------------------------------------- steps 2 - 3: gradients and their SADs
// sad[(j * KR + k) * (2R+1) + d + R].  The block's rows are dealt to its 16 waves; a lane owns offset index `lane` (lane 0 also index
// 64, which exists for R = 32 only).  The profiles are a few KB and stay in L2: G is recomputed from them where it is needed.
constexpr int AL_SAD_WAVES = 16;
__global__ __launch_bounds__(64 * AL_SAD_WAVES) void stm_k_align_sad(uint32_t *__restrict__ sad, const uint32_t *__restrict__ prof, int H, int R)
{
    __shared__ uint32_t part[AL_SAD_WAVES][2 * AL_RMAX + 1];
    const int j = blockIdx.x, k = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nd = 2 * R + 1;
    const int r0 = (int)((long long)k * H / AL_KR), r1 = (int)((long long)(k + 1) * H / AL_KR);
    const uint32_t *__restrict__ pl = prof + (size_t)j * H, *__restrict__ pr = prof + ((size_t)AL_KB + j) * H;
    uint32_t acc[2] = {0, 0};
    for (int y = r0 + wave; y < r1; y += AL_SAD_WAVES) {
        const int gl = (int)(pl[min(y + 1, H - 1)] - pl[max(y - 1, 0)]);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int di = lane + 64 * i;
            if (di >= nd) continue;
            const int yy = min(max(y + di - R, 0), H - 1);
            const int gr = (int)(pr[min(yy + 1, H - 1)] - pr[max(yy - 1, 0)]);
            acc[i] += (uint32_t)abs(gl - gr);
        }
    }
    part[wave][lane] = acc[0];
    if (lane == 0) part[wave][64] = acc[1];
    __syncthreads();
    if ((int)threadIdx.x < nd) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < AL_SAD_WAVES; ++w) sum += part[w][threadIdx.x];
        sad[((size_t)j * AL_KR + k) * nd + threadIdx.x] = sum;
    }
}

// ---------------------------------------------------------------- steps 4 - 6: the fit
constexpr int AL_NB = AL_KB * AL_KR;
struct AlignFitArgs {
    int H, W, R;
    float rate;
    int fresh; // the state's history is ignored (a null d_state: every frame fitted on its own)
};
// The weighted plane through the blocks of weight > 0 (stm_hip.h): the normal equations summed in block order and solved by Cramer's
// rule, f64, one operation per line (the file is compiled -ffp-contract=off; the f64 division is the correctly rounded one).
// Returns 0 when no block has weight.
__device__ int align_solve(const double *wt, const double *o, const double *uc, const double *vc, double x[3])
{
    int n = 0;
    double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0, t, p;
    for (int i = 0; i < AL_NB; ++i) {
        if (!(wt[i] > 0.0)) continue;
        ++n;
        const double wi = wt[i], u = uc[i], v = vc[i], oi = o[i];
        const double wu = wi * u;
        const double wv = wi * v;
        m00 = m00 + wi;
        m01 = m01 + wu;
        m02 = m02 + wv;
        t = wu * u;
        m11 = m11 + t;
        t = wu * v;
        m12 = m12 + t;
        t = wv * v;
        m22 = m22 + t;
        t = wi * oi;
        r0 = r0 + t;
        t = wu * oi;
        r1 = r1 + t;
        t = wv * oi;
        r2 = r2 + t;
    }
    if (n == 0) return 0;
    t = m11 * m22;
    p = m12 * m12;
    const double c00 = t - p;
    t = m01 * m22;
    p = m12 * m02;
    const double c01 = t - p;
    t = m01 * m12;
    p = m11 * m02;
    const double c02 = t - p;
    t = m00 * c00;
    p = m01 * c01;
    double det = t - p;
    p = m02 * c02;
    det = det + p;
    double bound = m00 * m11;
    bound = bound * m22;
    bound = 1.0e-6 * bound;
    if (n < 3 || !(det > bound)) { // no plane is determined: the weighted mean
        x[0] = r0 / m00;
        x[1] = 0.0;
        x[2] = 0.0;
        return 1;
    }
    t = m00 * m22;
    p = m02 * m02;
    const double c11 = t - p;
    t = m00 * m12;
    p = m01 * m02;
    const double c12 = t - p;
    t = m00 * m11;
    p = m01 * m01;
    const double c22 = t - p;
    t = c00 * r0;
    p = c01 * r1;
    t = t - p;
    p = c02 * r2;
    t = t + p;
    x[0] = t / det;
    t = c11 * r1;
    p = c01 * r0;
    t = t - p;
    p = c12 * r2;
    t = t - p;
    x[1] = t / det;
    t = c02 * r0;
    p = c12 * r1;
    t = t - p;
    p = c22 * r2;
    t = t + p;
    x[2] = t / det;
    return 1;
}

// One wave.  Lane i < 32 owns block i = j * KR + k: the scan for its minimum, its offset and weight.  Lane 0 then fits and updates
// the state {valid, a, b, c}; nvalid (may be null) receives the number of valid blocks.
__global__ __launch_bounds__(64) void stm_k_align_fit(float *__restrict__ state, int *__restrict__ nvalid, const uint32_t *__restrict__ sad,
                                                      AlignFitArgs a)
{
    __shared__ double s_o[AL_NB], s_w[AL_NB], s_w2[AL_NB], s_uc[AL_NB], s_vc[AL_NB];
    const int lane = threadIdx.x, R = a.R, nd = 2 * R + 1;
    bool valid = false;
    if (lane < AL_NB) {
        const uint32_t *__restrict__ s = sad + (size_t)lane * nd;
        uint32_t best = s[R];
        int bi = R;
        long long tot = s[R];
        for (int m = 1; m <= R; ++m) { // d = 0, -1, +1, -2, +2, ...: strict less-than, ties go to the smaller |d|
            const uint32_t lo = s[R - m], hi = s[R + m];
            tot += (long long)lo + (long long)hi;
            if (lo < best) { best = lo; bi = R - m; }
            if (hi < best) { best = hi; bi = R + m; }
        }
        double o = 0.0, w = 0.0;
        if (bi != 0 && bi != nd - 1) {
            const long long sm = s[bi - 1], sc = s[bi], sp = s[bi + 1];
            const long long den = sm - 2 * sc + sp;
            if (den > 0) {
                valid = true;
                const double num = (double)(sm - sp);
                double t = num / (double)den;
                t = 0.5 * t;
                o = (double)(bi - R) + t;
                t = (double)den * (double)nd;
                w = t / (double)(tot > 1 ? tot : 1);
            }
        }
        const int j = lane / AL_KR, k = lane % AL_KR;
        const long long x0 = (long long)j * a.W / AL_KB, x1 = (long long)(j + 1) * a.W / AL_KB;
        const long long y0 = (long long)k * a.H / AL_KR, y1 = (long long)(k + 1) * a.H / AL_KR;
        double t = (double)(x0 + x1 - 1) * 0.5;
        double c = (double)(a.W - 1) * 0.5;
        s_uc[lane] = t - c;
        t = (double)(y0 + y1 - 1) * 0.5;
        c = (double)(a.H - 1) * 0.5;
        s_vc[lane] = t - c;
        s_o[lane] = o;
        s_w[lane] = w;
    }
    const int count = __popcll(__ballot(valid));
    __syncthreads();
    if (lane != 0) return;
    if (nvalid) *nvalid = count;
    const bool start = a.fresh || state[0] == 0.0f;
    double x[3], y[3];
    if (!align_solve(s_w, s_o, s_uc, s_vc, x)) { // no valid block: the state is kept; one without a history gets zeros
        if (start) {
            state[0] = 0.0f; state[1] = 0.0f; state[2] = 0.0f; state[3] = 0.0f;
        }
        return;
    }
    for (int i = 0; i < AL_NB; ++i) { // blocks more than a row off the plane lose their weight, and the plane is fitted once more
        double t = x[1] * s_uc[i];
        double e = x[0] + t;
        t = x[2] * s_vc[i];
        e = e + t;
        e = s_o[i] - e;
        s_w2[i] = (s_w[i] > 0.0 && !(fabs(e) > 1.0)) ? s_w[i] : 0.0;
    }
    if (align_solve(s_w2, s_o, s_uc, s_vc, y)) { x[0] = y[0]; x[1] = y[1]; x[2] = y[2]; }
    if (start) {
        state[0] = 1.0f;
        state[1] = (float)x[0];
        state[2] = (float)x[1];
        state[3] = (float)x[2];
        return;
    }
    for (int i = 0; i < 3; ++i) {
        const double old = (double)state[1 + i];
        double t = x[i] - old;
        t = (double)a.rate * t;
        state[1 + i] = (float)(old + t);
    }
}

// ---------------------------------------------------------------- apply
// One thread per pixel of the output row: columns [0, first_right) are the left eye, copied; the rest the right eye, sampled at row
// y + dy.  The stage call has first_right = 0 and one image as eye 1.  state != nullptr: a, b, c are read from {valid, a, b, c}.
struct AlignField {
    float a, b, c;
    const float *state;
};
template <int FMT, int AXIS, int FILT>
__global__ __launch_bounds__(256) void stm_k_align_frame(u8 *__restrict__ out, AlignSrc s, AlignField fld, int H, int W, int first_right,
                                                         int out_cols)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= out_cols) return;
    uint32_t px;
    if (x < first_right) {
        px = al_unpacked_px<FMT, AXIS, FILT>(s, 0, y, x);
    } else {
        const int ex = x - first_right;
        const float a = fld.state ? fld.state[1] : fld.a, b = fld.state ? fld.state[2] : fld.b, c = fld.state ? fld.state[3] : fld.c;
        const float u = (float)ex - 0.5f * (float)(W - 1), v = (float)y - 0.5f * (float)(H - 1);
        float t = b * u;
        float sm = a + t;
        t = c * v;
        sm = sm + t;
        float m = sm * 16.0f;
        m = m + 0.5f;
        m = floorf(m);
        m = fminf(fmaxf(m, -1024.0f), 1024.0f);
        const int q = (int)m, ya = y + (q >> 4), f = q & 15;
        const uint32_t pa = al_unpacked_px<FMT, AXIS, FILT>(s, 1, min(max(ya, 0), H - 1), ex);
        px = pa;
        if (f) {
            const uint32_t pb = al_unpacked_px<FMT, AXIS, FILT>(s, 1, min(max(ya + 1, 0), H - 1), ex);
            px = 0;
#pragma unroll
            for (int ch = 0; ch < 24; ch += 8)
                px |= (uint32_t)(((16 - f) * (int)((pa >> ch) & 0xff) + f * (int)((pb >> ch) & 0xff) + 8) >> 4) << ch;
        }
    }
    u8 *d = out + ((size_t)y * out_cols + x) * s.elem_sz;
    d[0] = (u8)px; d[1] = (u8)(px >> 8); d[2] = (u8)(px >> 16);
}

struct ProfilesLaunch {
    uint32_t *prof;
    AlignSrc s;
    int H, W;
    template <int FMT, int AXIS, int FILT> void run() const
    {
        const long long segs = 2ll * H * AL_KB;
        STM_LAUNCH((stm_k_align_profiles<FMT, AXIS, FILT>), dim3((unsigned)((segs + 3) / 4)), dim3(256), 0, stream(), prof, s, H, W);
    }
};
struct FrameLaunch {
    u8 *out;
    AlignSrc s;
    AlignField fld;
    int H, W, first_right, out_cols;
    template <int FMT, int AXIS, int FILT> void run() const
    {
        STM_LAUNCH((stm_k_align_frame<FMT, AXIS, FILT>), dim3(cdiv(out_cols, 256), H), dim3(256), 0, stream(), out, s, fld, H, W, first_right,
                   out_cols);
    }
};

} // namespace

size_t align_profile_words(int H) { return (size_t)2 * AL_KB * H; }
size_t align_sad_words(int radius) { return (size_t)AL_NB * (2 * radius + 1); }

void launch_align_measure(float *state, int *nvalid, uint32_t *prof, uint32_t *sad, const PackInput *in, const u8 *img_l, const u8 *img_r,
                          int H, int W, int elem_sz, int radius, float rate, bool fresh)
{
    {
        ProfScope p("align_profiles");
        dispatch(in, ProfilesLaunch{prof, make_src(in, img_l, img_r, H, W, elem_sz), H, W});
        STM_CHECK_LAUNCH();
    }
    {
        ProfScope p("align_sad");
        STM_LAUNCH(stm_k_align_sad, dim3(AL_KB, AL_KR), dim3(64 * AL_SAD_WAVES), 0, stream(), sad, prof, H, radius);
        STM_CHECK_LAUNCH();
    }
    ProfScope p("align_fit");
    const AlignFitArgs a{H, W, radius, rate, fresh ? 1 : 0};
    STM_LAUNCH(stm_k_align_fit, dim3(1), dim3(64), 0, stream(), state, nvalid, sad, a);
    STM_CHECK_LAUNCH();
}

void launch_align_frame(u8 *out, const PackInput *in, const u8 *img, int H, int W, int elem_sz, float a, float b, float c, const float *state)
{
    ProfScope p("align_frame");
    const AlignField fld{a, b, c, state};
    dispatch(in, FrameLaunch{out, make_src(in, img, img, H, W, elem_sz), fld, H, W, in ? W : 0, in ? 2 * W : W});
    STM_CHECK_LAUNCH();
}

} // namespace stm
