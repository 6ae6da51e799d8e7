// What does an exact window sum cost as a run of vector adds, lane = hypothesis?  The inner structure planned for the vertical
// aggregation kernel, with nothing around it.  Per run (= one window of one pass): a table entry (scalar load, a run ahead) gives
// the window length L and a ring index; the index mode is switched on (src0 relative), one computed jump (s_swappc_b64) enters a
// straight sequence of 72 dependent `v_add_f32 vacc, v[ring + j], vacc` at 72 - L, the sequence returns through a register pair,
// and one v_mov with a relative destination puts a row into the ring.  L is uniform over [0, 48] (mean 24), or over the range
// given as two arguments (0 0 and 72 72 separate a run's fixed cost from the cost of an add).
// MEM = 0: no memory access.  MEM = 1: one buffer_load_dword (256 bytes per wave, nt, sixteen rows ahead) and one
// buffer_store_dword per run.  MEM = 2: one of each per TWO runs, the kernel's own ratio (two passes per row).  A wave owns a column
// of a pixel-major volume: consecutive rows lie NW * 256 bytes apart, NW = waves of the launch.  Two diagnoses of the add rate
// (two chains in turn; the same adds with the index mode off), then k_probe_abs: the same sums with every register named.
//   hipcc --offload-arch=gfx950 -O3 tools/vadd_chain_probe.hip -o /tmp/vcp && /tmp/vcp
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

constexpr int RUNS = 2048; // runs per wave = entries of the table = rows of the probe's volumes (a multiple of 16)

// Register map: v0 accumulator, v1 load offset (4 lane), v2 store offset, v[8:111] the registers a run can read (the sequence names
// v[8:79], the index adds 0 .. 32), v[112:127] landing registers: 128 registers, so that four waves per SIMD are resident (the add
// rate does not depend on WHICH registers a run reads; the kernel's two rings of 72 need more).  s[16:19] / s[20:23] buffer
// descriptors, s24 table offset, s25 row offset of the loads, s26 of the stores, s27 table entry (in flight), s28 entry offset, s29 ring index, s[30:31] jump target,
// s[36:37] start of the sequence, s[38:39] return address.
template <int MEM>
__global__ __launch_bounds__(256) void k_probe(const float *in, float *out, const uint32_t *tab, int nw)
{
    const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rsb = nw * 256;
    const uint32_t range = (uint32_t)(RUNS - 1) * (uint32_t)rsb + 256u; // bytes of a column up to the end of its last row
    const float *cin = in + (size_t)w * 64;
    float *cout = out + (size_t)w * 64;
    asm volatile(R"ASM(
        .set VP_MEM, %[mem]
        .macro VP_RUN k
        s_waitcnt lgkmcnt(0)                  ; this run's entry, requested a run ago
        s_and_b32 s28, s27, 0xffff
        s_lshr_b32 s29, s27, 16
        s_load_dword s27, %[tab], s24
        s_add_u32 s24, s24, 4
        s_add_u32 s30, s36, s28
        s_addc_u32 s31, s37, 0
        .if (VP_MEM == 1) || ((VP_MEM == 2) && (((\k) & 1) == 0))
        .if VP_MEM == 1
        s_waitcnt vmcnt(31)                   ; the load of sixteen runs ago (issued since: 15 loads, 16 stores)
        .else
        s_waitcnt vmcnt(15)
        .endif
        .endif
        v_mov_b32 v0, 0
        s_set_gpr_idx_on s29, 0x8
        v_mov_b32 v8, v[112+\k]               ; a row enters the ring
        .if (VP_MEM == 1) || ((VP_MEM == 2) && (((\k) & 1) == 0))
        buffer_load_dword v[112+\k], v1, s[16:19], s25 offen nt
        s_add_u32 s25, s25, %[rsb]
        .endif
        .if VP_MEM == 4
        s_set_gpr_idx_off                     ; (diagnosis only: the same adds with the index mode off)
        .else
        s_set_gpr_idx_mode 0x1
        .endif
        s_swappc_b64 s[38:39], s[30:31]
        s_set_gpr_idx_off
        .if (VP_MEM == 1) || ((VP_MEM == 2) && (((\k) & 1) == 0))
        buffer_store_dword v0, v2, s[20:23], s26 offen nt
        s_add_u32 s26, s26, %[rsb]
        .endif
        .endm

        s_mov_b64 s[16:17], %[in]
        s_and_b32 s17, s17, 0xffff
        s_mov_b32 s18, %[range]
        s_mov_b32 s19, 0x20000
        s_mov_b64 s[20:21], %[out]
        s_and_b32 s21, s21, 0xffff
        s_mov_b32 s22, %[range]
        s_mov_b32 s23, 0x20000
        v_mbcnt_lo_u32_b32 v3, -1, 0
        v_mbcnt_hi_u32_b32 v3, -1, v3         ; lane 16 b + n
        v_lshlrev_b32 v1, 2, v3               ; loads float 16 b + n
        v_and_b32 v2, 15, v3
        v_lshrrev_b32 v3, 4, v3
        v_lshl_add_u32 v2, v2, 2, v3
        v_lshlrev_b32 v2, 2, v2               ; and stores at float 4 n + b
        .set VP_i, 8
        .rept 120
        v_mov_b32 v[VP_i], 1.0
        .set VP_i, VP_i+1
        .endr
        s_mov_b32 s24, 4
        s_mov_b32 s25, 0
        s_mov_b32 s26, 0
        s_load_dword s27, %[tab], 0x0
        s_getpc_b64 s[36:37]
VP_pc_%=:
        s_add_u32 s36, s36, VP_seq_%=-VP_pc_%=
        s_addc_u32 s37, s37, 0
        s_branch VP_loop_%=
VP_seq_%=:
        .set VP_i, 8
        .rept 36
        v_add_f32 v0, v[VP_i], v0
        .if VP_MEM == 3
        v_add_f32 v3, v[VP_i+1], v3           ; (diagnosis only: two chains in turn -- is it the dependency that costs?)
        .else
        v_add_f32 v0, v[VP_i+1], v0
        .endif
        .set VP_i, VP_i+2
        .endr
VP_seqend_%=:
        .if (VP_seqend_%=-VP_seq_%=) != 72*4
        .error "an add of the sequence is not 4 bytes"
        .endif
        s_setpc_b64 s[38:39]
VP_loop_%=:
        VP_RUN 0
        VP_RUN 1
        VP_RUN 2
        VP_RUN 3
        VP_RUN 4
        VP_RUN 5
        VP_RUN 6
        VP_RUN 7
        VP_RUN 8
        VP_RUN 9
        VP_RUN 10
        VP_RUN 11
        VP_RUN 12
        VP_RUN 13
        VP_RUN 14
        VP_RUN 15
        s_cmp_lt_u32 s24, %[tend]
        s_cbranch_scc1 VP_loop_%=
        s_waitcnt vmcnt(0) lgkmcnt(0)
        .purgem VP_RUN
        )ASM"
                 :
                 : [in] "s"(cin), [out] "s"(cout), [tab] "s"(tab), [rsb] "s"(rsb), [range] "s"(range), [tend] "s"(4 * RUNS), [mem] "n"(MEM)
                 : "memory", "scc", "vcc", "m0",
                   "s16", "s17", "s18", "s19", "s20", "s21", "s22", "s23", "s24", "s25", "s26", "s27", "s28", "s29", "s30", "s31", "s36", "s37", "s38", "s39",
                   "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19",
                   "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39",
                   "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59",
                   "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79",
                   "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99",
                   "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116",
                   "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127");
}

// The same sums with NO index mode: every register is named.  A window that ends at ring position e is summed by sequence e of its
// ring, the 72 adds over positions e - 71 .. e (mod 72), entered at 72 - L: 72 sequences of 292 bytes per ring, 42 KB for the two
// rings, and a window that crosses the ring's end needs no second run.  The table entry is the entry's byte offset (low half) and
// the ring index of the row that enters (high half; the v_mov into the ring keeps the index mode).  Each wave starts at its own
// place in the table, so that the waves of a CU are spread over the sequences as the columns of an image would be.
// Register map: v0 accumulator, v1 / v2 offsets, v[8:79] ring 1, v[80:151] ring 2, v[152:167] landing registers; scalars as above,
// s40 runs left.
template <int MEM>
__global__ __launch_bounds__(256) void k_probe_abs(const float *in, float *out, const uint32_t *tab, int nw)
{
    const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rsb = nw * 256;
    const uint32_t range = (uint32_t)(RUNS - 1) * (uint32_t)rsb + 256u;
    const float *cin = in + (size_t)w * 64;
    float *cout = out + (size_t)w * 64;
    const int t0 = 4 * ((w * 37) & (RUNS - 1));
    asm volatile(R"ASM(
        .set VA_MEM, %[mem]
        .macro VA_RUN k
        s_waitcnt lgkmcnt(0)                  ; this run's entry, requested a run ago
        s_and_b32 s28, s27, 0xffff
        s_lshr_b32 s29, s27, 16
        s_load_dword s27, %[tab], s24
        s_add_u32 s24, s24, 4
        s_and_b32 s24, s24, %[tmask]
        s_add_u32 s30, s36, s28
        s_addc_u32 s31, s37, 0
        .if (VA_MEM == 2) && (((\k) & 1) == 0)
        s_waitcnt vmcnt(15)                   ; the load of sixteen runs ago (issued since: 7 loads, 8 stores)
        .endif
        v_mov_b32 v0, 0
        s_set_gpr_idx_on s29, 0x8
        v_mov_b32 v8, v[152+\k]               ; a row enters a ring
        s_set_gpr_idx_off
        .if (VA_MEM == 2) && (((\k) & 1) == 0)
        buffer_load_dword v[152+\k], v1, s[16:19], s25 offen nt
        s_add_u32 s25, s25, %[rsb]
        .endif
        s_swappc_b64 s[38:39], s[30:31]
        .if (VA_MEM == 2) && (((\k) & 1) == 0)
        buffer_store_dword v0, v2, s[20:23], s26 offen nt
        s_add_u32 s26, s26, %[rsb]
        .endif
        .endm

        s_mov_b64 s[16:17], %[in]
        s_and_b32 s17, s17, 0xffff
        s_mov_b32 s18, %[range]
        s_mov_b32 s19, 0x20000
        s_mov_b64 s[20:21], %[out]
        s_and_b32 s21, s21, 0xffff
        s_mov_b32 s22, %[range]
        s_mov_b32 s23, 0x20000
        v_mbcnt_lo_u32_b32 v3, -1, 0
        v_mbcnt_hi_u32_b32 v3, -1, v3         ; lane 16 b + n
        v_lshlrev_b32 v1, 2, v3               ; loads float 16 b + n
        v_and_b32 v2, 15, v3
        v_lshrrev_b32 v3, 4, v3
        v_lshl_add_u32 v2, v2, 2, v3
        v_lshlrev_b32 v2, 2, v2               ; and stores at float 4 n + b
        .set VA_i, 8
        .rept 160
        v_mov_b32 v[VA_i], 1.0
        .set VA_i, VA_i+1
        .endr
        s_mov_b32 s25, 0
        s_mov_b32 s26, 0
        s_mov_b32 s40, %[runs]
        s_load_dword s27, %[tab], %[t0]
        s_add_u32 s24, %[t0], 4
        s_and_b32 s24, s24, %[tmask]
        s_getpc_b64 s[36:37]
VA_pc_%=:
        s_add_u32 s36, s36, VA_seq_%=-VA_pc_%=
        s_addc_u32 s37, s37, 0
        s_branch VA_loop_%=
VA_seq_%=:
        .set VA_rb, 8
        .rept 2
        .set VA_e, 0
        .rept 72
        .set VA_j, 0
        .rept 72
        v_add_f32 v0, v[VA_rb+(VA_e+1+VA_j)%%72], v0
        .set VA_j, VA_j+1
        .endr
        s_setpc_b64 s[38:39]
        .set VA_e, VA_e+1
        .endr
        .set VA_rb, VA_rb+72
        .endr
VA_seqend_%=:
        .if (VA_seqend_%=-VA_seq_%=) != 144*292
        .error "a sequence is not 292 bytes"
        .endif
VA_loop_%=:
        VA_RUN 0
        VA_RUN 1
        VA_RUN 2
        VA_RUN 3
        VA_RUN 4
        VA_RUN 5
        VA_RUN 6
        VA_RUN 7
        VA_RUN 8
        VA_RUN 9
        VA_RUN 10
        VA_RUN 11
        VA_RUN 12
        VA_RUN 13
        VA_RUN 14
        VA_RUN 15
        s_sub_u32 s40, s40, 16
        s_cmp_lg_u32 s40, 0
        s_cbranch_scc1 VA_loop_%=
        s_waitcnt vmcnt(0) lgkmcnt(0)
        .purgem VA_RUN
        )ASM"
                 :
                 : [in] "s"(cin), [out] "s"(cout), [tab] "s"(tab), [rsb] "s"(rsb), [range] "s"(range), [runs] "s"(RUNS), [t0] "s"(t0), [tmask] "s"(4 * RUNS - 1), [mem] "n"(MEM)
                 : "memory", "scc", "vcc", "m0",
                   "s16", "s17", "s18", "s19", "s20", "s21", "s22", "s23", "s24", "s25", "s26", "s27", "s28", "s29", "s30", "s31", "s36", "s37", "s38", "s39", "s40",
                   "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19",
                   "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39",
                   "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59",
                   "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79",
                   "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99",
                   "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116",
                   "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143",
                   "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160",
                   "v161", "v162", "v163", "v164", "v165", "v166", "v167");
}

template <int MEM, bool ABS = false> static void run(const float *din, float *dout, const uint32_t *tab, double mean_l, int wps, const char *what)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const int nblk = 256 * wps, nw = 4 * nblk; // block = 4 waves = one per SIMD; wps blocks per CU
    float best = 1e30f, worst = 0.f;
    for (int r = 0; r < 5; ++r) {
        CK(hipEventRecord(e0, 0));
        if (ABS) hipLaunchKernelGGL((k_probe_abs<MEM>), dim3(nblk), dim3(256), 0, 0, din, dout, ABS ? tab + RUNS + 16 : tab, nw);
        else hipLaunchKernelGGL((k_probe<MEM>), dim3(nblk), dim3(256), 0, 0, din, dout, tab, nw);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r == 0) continue; // the first launch loads the code
        if (ms < best) best = ms;
        if (ms > worst) worst = ms;
    }
    const double cyc = best * 1e-3 * 2.4e9 / ((double)RUNS * wps), cycw = worst * 1e-3 * 2.4e9 / ((double)RUNS * wps);
    const double nrows = (double)RUNS / (MEM == 2 ? 2 : 1);
    printf("%-34s waves/SIMD %d: %6.1f cycles per run per SIMD at 2.4 GHz (slowest of 4: %6.1f) = %.2f per add", what, wps, cyc, cycw, mean_l > 0 ? cyc / mean_l : 0.0);
    if (MEM == 1 || MEM == 2) printf(", %.2f TB/s", 2.0 * nrows * 256.0 * nw / (best * 1e-3) * 1e-12);
    printf("\n");
}

int main(int argc, char **argv)
{
    const uint32_t lmin = argc > 2 ? atoi(argv[1]) : 0, lmax = argc > 2 ? atoi(argv[2]) : 48; // window lengths: uniform over [lmin, lmax]
    std::vector<uint32_t> h(2 * RUNS + 16); // the table of the indexed form, then that of the named-register form
    uint32_t s = 12345u;
    double sum = 0;
    for (int i = 0; i < RUNS + 16; ++i) {
        s = s * 1664525u + 1013904223u;
        const uint32_t L = lmin + (s >> 8) % (lmax - lmin + 1u);
        s = s * 1664525u + 1013904223u;
        const uint32_t idx = (s >> 8) % 33u;
        h[i] = (4u * (72u - L)) | (idx << 16);
        if (i < RUNS) sum += L;
    }
    for (int i = 0; i < RUNS; ++i) { // the same lengths; a sequence (ring and end position) and a ring index drawn for each
        s = s * 1664525u + 1013904223u;
        const uint32_t e = (s >> 8) % 144u, L = 72u - (h[i] & 0xffffu) / 4u;
        s = s * 1664525u + 1013904223u;
        h[RUNS + 16 + i] = (292u * e + 4u * (72u - L)) | (((s >> 8) % 144u) << 16);
    }
    const double mean_l = sum / RUNS;
    printf("# %d runs per wave, lengths uniform over [%u, %u], mean %.2f adds\n", RUNS, lmin, lmax, mean_l);
    uint32_t *tab;
    CK(hipMalloc(&tab, h.size() * 4));
    CK(hipMemcpy(tab, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    const size_t vol = (size_t)RUNS * (4 * 256 * 4) * 256; // rows x the most waves of a launch x 256 bytes
    float *din, *dout;
    CK(hipMalloc(&din, vol));
    CK(hipMalloc(&dout, vol));
    CK(hipMemset(din, 0, vol));
    CK(hipMemset(dout, 0, vol));
    for (int wps = 1; wps <= 4; ++wps) run<0>(din, dout, tab, mean_l, wps, "adds only");
    for (int wps = 1; wps <= 4; ++wps) run<3>(din, dout, tab, mean_l, wps, "adds only, two chains in turn");
    for (int wps = 1; wps <= 4; ++wps) run<4>(din, dout, tab, mean_l, wps, "adds only, index mode off");
    for (int wps = 2; wps <= 3; ++wps) run<1>(din, dout, tab, mean_l, wps, "+ a load and a store per run");
    for (int wps = 2; wps <= 3; ++wps) run<2>(din, dout, tab, mean_l, wps, "+ a load and a store per two runs");
    for (int wps = 1; wps <= 3; ++wps) run<0, true>(din, dout, tab, mean_l, wps, "named registers: adds only");
    for (int wps = 2; wps <= 3; ++wps) run<2, true>(din, dout, tab, mean_l, wps, "named: + load, store per two runs");
    CK(hipDeviceSynchronize());
    return 0;
}
