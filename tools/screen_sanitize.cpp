// screen_sanitize.cpp -- the argument screens under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU and without Python:
// a few dozen calls that the entries refuse before they touch the device (error mode 1), through every kind of refusal the host
// layer has -- the printf-checked helper with each of its conversions (%d, %g, %s, %zu, %lld, %llu, 0x%x), the null-pointer rule
// with one, two and three names, the literal messages of the setters, the longest messages of the library.  Built and run by
// tools/screen_sanitize.sh, which compiles the library's host code with -Xarch_host -fsanitize=address,undefined; any report
// fails the run, and so does a call that is not refused or whose message does not begin with its entry's name.
#include "../include/stm_hip.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

static int g_bad = 0, g_calls = 0;

// the message after its first line (the fail site) must begin with "<name>: "
static void refused(const char *name)
{
    ++g_calls;
    const char *e = stm_last_error();
    const char *text = strchr(e, '\n');
    char want[128];
    snprintf(want, sizeof want, "%s: ", name);
    if (!text || strncmp(text + 1, want, strlen(want)) != 0) {
        fprintf(stderr, "screen_sanitize: expected a refusal by %s, stm_last_error() is:\n%s\n", name, e);
        ++g_bad;
    }
}

int main()
{
    stm_set_error_mode(1);
    unsigned char *p1 = (unsigned char *)0x100000, *p2 = (unsigned char *)0x200000, *p3 = (unsigned char *)0x300000; // never dereferenced
    float *f1 = (float *)0x400000, *f2 = (float *)0x500000, *f3 = (float *)0x600000;
    int *i1 = (int *)0x700000;
    const float nan = nanf(""), inf = INFINITY;
    int rect[4] = {0, 9, 0, 16};
    unsigned char lut[768];
    for (int i = 0; i < 768; ++i) lut[i] = (unsigned char)i;

    // the dimension screen, %s %s %d %d
    stm_d_filter_median(f1, 0, 16); refused("d_filter_median");
    stm_d_dc_wta((float **)f1, f2, 4, 2, -2147483647 - 1, 16); refused("d_dc_wta");
    stm_generate_gaussian_kernel(f1, -1, 1.0f); refused("generate_gaussian_kernel");
    // %g with NaN and infinities, %zu, %lld, %llu, 0x%x
    stm_d_disp_upsample(f1, f2, p1, p2, 8, 16, 4, 8, 3, 2.0f, nan); refused("d_disp_upsample");
    stm_d_disp_temporal(f1, f2, p1, p2, 8, 16, 3, inf, 30, 1.0f); refused("d_disp_temporal");
    stm_d_disp_temporal(f1, f1 + 1, p1, p2, 8, 16, 3, 0.5f, 30, 1.0f); refused("d_disp_temporal");
    stm_d_depth_fit(f1, f2, 65536, 32768, -2.0f, 2.0f, 4.0f, 20, 0.5f, f3); refused("d_depth_fit");
    stm_d_depth_fit_rect(f1, f2, 8, 16, -inf, nan, 4.0f, 20, 0.5f, f3, i1); refused("d_depth_fit_rect");
    stm_depth_fit_rect(f1, f2, 8, 16, -2.0f, 2.0f, 4.0f, 20, 0.5f, f3, rect); refused("depth_fit_rect");
    stm_d_align_fit(p1, p2, 2147483647, 2147483647, 3, 16, 1.0f, f1, i1, nullptr, nullptr); refused("d_align_fit");
    stm_d_demux_packed(p1, p2, p3, 8, 20, 16, 3, 1, 0, 0, 2147483647); refused("d_demux_packed");
    stm_d_demux_packed(p1, p2, p3, 8, 20, 16, 3, 1, 0, 0, 5); refused("d_demux_packed");
    stm_d_adcensus_stm_2s(p1, f1, f2, p2, 8, 32, 16, 8, 16, 4, 8, 3, 0.5f, 8, 18.43f, 4, 2, 10.0f, 30.0f, 20.0f, 6.0f, 5, 3, 20, 0.4f, 0x7fffffff);
    refused("d_adcensus_stm_2s");
    // the null-pointer rule: one, two and three names
    stm_d_active_fill(nullptr, 8, 16, i1, 0.0f); refused("d_active_fill");
    stm_d_align_rows(nullptr, p1, 8, 16, 3, 0.5f, 0.0f, 0.0f); refused("d_align_rows");
    stm_d_cut_detect(p1, 8, 16, 3, 370, 1, nullptr, nullptr, nullptr, nullptr, nullptr); refused("d_cut_detect");
    stm_d_balance_fit(nullptr, nullptr, 8, 16, 3, 48, 1.0f, nullptr, nullptr); refused("d_balance_fit");
    stm_d_view_prefilter(p1, p2, nullptr, 8, 16, 3, 8, 1.0f, 4, 0.5f, 1.0f, 0.0f); refused("d_view_prefilter");
    // overlaps, pairs of pointers
    stm_d_view_prefilter(p1, p1 + 383, f1, 8, 16, 3, 8, 1.0f, 4, 0.5f, 1.0f, 0.0f); refused("d_view_prefilter");
    stm_d_balance_apply(p1, p2, 8, 16, 3, lut, i1); refused("d_balance_apply");
    stm_d_demux_sbs_low(p1, p2, p3, p3, nullptr, (unsigned int *)f1, p1, 8, 32, 16, 4, 8, 3); refused("d_demux_sbs_low");
    // the longest messages: the packing and matrix sentences under the longest entry names, the quilt and the active rectangle
    stm_d_demux_nv12_packed(p1, p2, p3, 32, p3, 32, 8, 32, 16, 3, -2147483647 - 1, 0, 1, 0, 0); refused("d_demux_nv12_packed");
    stm_d_demux_nv12_packed(p1, p2, p3, 32, p3, 32, 8, 32, 16, 3, 0, -2147483647 - 1, 0, 0, 0); refused("d_demux_nv12_packed");
    stm_d_demux_nv12_packed(p1, p2, p3, 32, p3, 32, 2147483646, 2147483647, 2147483646, 3, 0, 3, 0, 0, 0); refused("d_demux_nv12_packed");
    stm_d_quilt_multiview((unsigned char **)p1, p2, 2147483647, 65535, 65535, 0, 0, 8, 16, 8, 16, 3); refused("d_quilt_multiview");
    rect[0] = -2147483647 - 1; rect[1] = -2147483647; rect[2] = -2147483647 - 1; rect[3] = -2147483647;
    stm_overlay_fit_rect(f1, f2, 2147483647, 1, p1, 2, 2, 0, 0, 8, 16, 1.0f, 0.0f, 20, 1.0f, 8, -4.0f, 4.0f, 1.0f, 0.1f, 0, f3, rect);
    refused("overlay_fit_rect");
    stm_d_mux_overlay(p1, p2, 2, 2, 0, 0, 0.0f, 8, 18.43f, 3, 5.0, 0.3, 0.0, 1, 4, 2, 0, 8, 16, 3); refused("d_mux_overlay");
    stm_d_mux_multiview((unsigned char **)p1, p2, 8, 0.0f, 8, 16, 8, 16, 3); refused("mux_multiview"); // (the geometry rule speaks as mux_multiview)
    // the thread setters: -1 and the setting untouched
    int before[4], after[4];
    stm_get_packing(before);
    if (stm_set_packing(4, 0, 0, 0) != -1) ++g_bad; refused("set_packing");
    if (stm_set_lens(1, nan, 0.3, 0.0) != -1) ++g_bad; refused("set_lens");
    if (stm_set_layout(1, 0, 2, 0, 0) != -1) ++g_bad; refused("set_layout");
    if (stm_set_output(1, 4, 0, 0) != -1) ++g_bad; refused("set_output");
    if (stm_set_overlay(1, p1 + 2, 2, 2, 0, 0, 0.0f) != -1) ++g_bad; refused("set_overlay");
    if (stm_set_overlay_auto(1, 20, 1.0f, 8, 2.0f, 1.0f, 1.0f, 0.1f, nullptr) != -1) ++g_bad; refused("set_overlay_auto");
    if (stm_set_depth(2, 1.0f, 0.0f) != -1) ++g_bad; refused("set_depth");
    if (stm_set_depth_auto(inf, -inf, 4.0f, 20, 0.5f, nullptr) != -1) ++g_bad; refused("set_depth_auto");
    if (stm_set_antialias(1, 1.0f, 17, 0.5f) != -1) ++g_bad; refused("set_antialias");
    if (stm_set_align(1, 0.0f, nan, 0.0f) != -1) ++g_bad; refused("set_align");
    if (stm_set_align_auto(33, 1.0f, nullptr) != -1) ++g_bad; refused("set_align_auto");
    if (stm_set_balance(1, nullptr) != -1) ++g_bad; refused("set_balance");
    if (stm_set_balance_auto(256, 1.0f, nullptr) != -1) ++g_bad; refused("set_balance_auto");
    if (stm_set_cut(1, 370, 1, nullptr) != -1) ++g_bad; refused("set_cut");
    if (stm_set_active(1, rect, 0, 0.0f) != -1) ++g_bad; refused("set_active");
    if (stm_set_active_auto(24, 10, 451, 12, nullptr) != -1) ++g_bad; refused("set_active_auto");
    if (stm_set_agg_tap(nullptr, (float *)(p1 + 2), nullptr, nullptr) != -1) ++g_bad; refused("set_agg_tap");
    if (stm_set_irv_chunk(17) != -1) ++g_bad; refused("set_irv_chunk");
    stm_get_packing(after);
    if (memcmp(before, after, sizeof before) != 0) ++g_bad;
    stm_set_error_mode(0);
    printf("screen_sanitize: %d refused calls, %d not as expected\n", g_calls, g_bad);
    return g_bad ? 1 : 0;
}
