/* oracle_map_edges.c -- runs the oracle's map-taking stages on the cases of tests/map_edge_cases.py, as a program of its own so
 * that the sanitizers see oracle/stm_oracle.c without a Python process around it:
 *
 *   gcc -O1 -g -fopenmp -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
 *       -o oracle_map_edges tools/oracle_map_edges.c oracle/stm_oracle.c -lm
 *   ./oracle_map_edges DIR
 *
 * DIR holds runs.txt and the raw files it names (tests/test_map_edges_ref.py writes them).  One run per line:
 *   pair H W N left.f32 right.f32          N map pairs: dr_dcc, dibr_occl, dibr_dfm (shifts 0, 0.4, 1, -1; 3 and 4 bytes per pixel)
 *                                          and filter_median on each map
 *   bilateral H W N D map.f32              N maps: filter_bilateral_1 with D table entries at radius 7 and 2
 *   irv H W N D zd usd disp.f32 outl.u8 cross.u8
 *                                          N maps and outlier maps over one table of arms [4][H][W]: dr_irv in both flavours,
 *                                          1 and 3 iterations, thresh_s 0 and 4, thresh_h 0 and 0.1, once more with the paper's ratio
 * The results are not compared here (test_map_edges_ref.py does that); a checksum keeps the calls alive.  Exit 0 and "ok:" on
 * stdout when every run finished; a sanitizer report ends the program with its own message on stderr. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef unsigned char u8;
void orc_set_irv_paper_ratio(int on);
void orc_dr_dcc(u8 *out_l, u8 *out_r, const float *disp_l, const float *disp_r, int H, int W);
void orc_dr_irv(float *disp, u8 *outl, const u8 *cross, int thresh_s, float thresh_h, int H, int W, int D, int zd, int usd,
                int iterations, int device_flavour);
void orc_filter_bilateral_1(float *img, int radius, float sigma_color, float sigma_spatial, int H, int W, int D);
void orc_filter_median(float *img, int H, int W);
void orc_dibr_occl(u8 *occl_l, u8 *occl_r, const float *disp_l, const float *disp_r, int H, int W);
void orc_dibr_dfm(u8 *img_out, const u8 *img_l, const u8 *img_r, const float *disp_l, const float *disp_r, float shift, int H,
                  int W, int elem_sz);

static void die(const char *what, const char *name)
{
    fprintf(stderr, "oracle_map_edges: %s %s\n", what, name);
    exit(2);
}

static void *slurp(const char *dir, const char *name, size_t bytes)
{
    char path[4096];
    snprintf(path, sizeof path, "%s/%s", dir, name);
    FILE *f = fopen(path, "rb");
    if (!f) die("cannot open", path);
    void *p = malloc(bytes ? bytes : 1);
    if (fread(p, 1, bytes, f) != bytes) die("short file", path);
    if (fgetc(f) != EOF) die("long file", path);
    fclose(f);
    return p;
}

static uint64_t sum_bytes(const void *p, size_t n)
{
    const u8 *b = (const u8 *)p;
    uint64_t s = 0;
    for (size_t i = 0; i < n; ++i) s = s * 31 + b[i];
    return s;
}

int main(int argc, char **argv)
{
    if (argc != 2) die("usage:", "oracle_map_edges DIR");
    const char *dir = argv[1];
    char path[4096], line[1024], kind[32], fa[256], fb[256], fc[256];
    snprintf(path, sizeof path, "%s/runs.txt", dir);
    FILE *runs = fopen(path, "r");
    if (!runs) die("cannot open", path);
    uint64_t sum = 0;
    long calls = 0;
    const float shifts[4] = {0.0f, 0.4f, 1.0f, -1.0f};
    while (fgets(line, sizeof line, runs)) {
        int H, W, N, D, zd, usd;
        if (sscanf(line, "%31s", kind) != 1) continue;
        if (!strcmp(kind, "pair")) {
            if (sscanf(line, "%*s %d %d %d %255s %255s", &H, &W, &N, fa, fb) != 5) die("bad line", line);
            const size_t HW = (size_t)H * W;
            float *l = (float *)slurp(dir, fa, HW * N * 4), *r = (float *)slurp(dir, fb, HW * N * 4);
            u8 *ol = (u8 *)malloc(HW), *orr = (u8 *)malloc(HW), *img = (u8 *)malloc(HW * 4), *out = (u8 *)malloc(HW * 4);
            float *m = (float *)malloc(HW * 4);
            for (size_t i = 0; i < HW * 4; ++i) img[i] = (u8)(1 + i % 255);
            for (int n = 0; n < N; ++n) {
                const float *dl = l + HW * n, *dr = r + HW * n;
                orc_dr_dcc(ol, orr, dl, dr, H, W);
                sum += sum_bytes(ol, HW) + sum_bytes(orr, HW);
                orc_dibr_occl(ol, orr, dl, dr, H, W);
                sum += sum_bytes(ol, HW) + sum_bytes(orr, HW);
                for (int s = 0; s < 4; ++s)
                    for (int e = 3; e <= 4; ++e) {
                        orc_dibr_dfm(out, img, img, dl, dr, shifts[s], H, W, e);
                        sum += sum_bytes(out, HW * e);
                    }
                for (int v = 0; v < 2; ++v) {
                    memcpy(m, v ? dr : dl, HW * 4);
                    orc_filter_median(m, H, W);
                    sum += sum_bytes(m, HW * 4);
                }
                calls += 14;
            }
            free(l); free(r); free(ol); free(orr); free(img); free(out); free(m);
        } else if (!strcmp(kind, "bilateral")) {
            if (sscanf(line, "%*s %d %d %d %d %255s", &H, &W, &N, &D, fa) != 5) die("bad line", line);
            const size_t HW = (size_t)H * W;
            float *l = (float *)slurp(dir, fa, HW * N * 4), *m = (float *)malloc(HW * 4);
            for (int n = 0; n < N; ++n)
                for (int k = 0; k < 2; ++k) {
                    memcpy(m, l + HW * n, HW * 4);
                    if (k == 0) orc_filter_bilateral_1(m, 7, 5.0f, 10.0f, H, W, D);
                    else orc_filter_bilateral_1(m, 2, 1.5f, 1.0f, H, W, D);
                    sum += sum_bytes(m, HW * 4);
                    ++calls;
                }
            free(l); free(m);
        } else if (!strcmp(kind, "irv")) {
            if (sscanf(line, "%*s %d %d %d %d %d %d %255s %255s %255s", &H, &W, &N, &D, &zd, &usd, fa, fb, fc) != 9) die("bad line", line);
            const size_t HW = (size_t)H * W;
            float *disp = (float *)slurp(dir, fa, HW * N * 4), *m = (float *)malloc(HW * 4);
            u8 *outl = (u8 *)slurp(dir, fb, HW * N), *cross = (u8 *)slurp(dir, fc, HW * 4), *o = (u8 *)malloc(HW);
            for (int n = 0; n < N; ++n)
                for (int k = 0; k < 17; ++k) { /* bits of k: flavour, iterations, thresh_s, thresh_h; k = 16: the paper's ratio */
                    memcpy(m, disp + HW * n, HW * 4);
                    memcpy(o, outl + HW * n, HW);
                    orc_set_irv_paper_ratio(k == 16);
                    orc_dr_irv(m, o, cross, (k & 4) ? 4 : 0, (k & 8) ? 0.1f : 0.0f, H, W, D, zd, usd, (k & 2) ? 3 : 1, k & 1);
                    sum += sum_bytes(m, HW * 4) + sum_bytes(o, HW);
                    ++calls;
                }
            orc_set_irv_paper_ratio(0);
            free(disp); free(m); free(outl); free(cross); free(o);
        } else {
            die("unknown run", kind);
        }
    }
    fclose(runs);
    printf("ok: %ld calls, checksum %016llx\n", calls, (unsigned long long)sum);
    return 0;
}
