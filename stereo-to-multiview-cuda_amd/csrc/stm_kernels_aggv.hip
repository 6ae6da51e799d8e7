// stm_kernels_aggv.hip -- both vertical aggregation passes of the frame pipeline, the rows of a strip held in REGISTERS.
//
// Reference stage replaced: ca_cross_vhsum_kernel_2 x 2 + both transposes,
// d_ca_cross_sum.cu:148-198 (window [y - armU, y + armD), ascending float32 adds), order d_ca_cross.cu:258-267.
//
// Round 3's fused vertical kernel (stm_k_pq_v12t, stm_kernels_aggm.hip) streams a strip through two LDS rings shared by the
// six waves of a block, two barriers per step; its matrix pipe was busy 48 % of the time (profiles/r03_pmc_sq_aggm.txt).
// Three kernels.  stm_k_pq_v12q (first below, round 4; PQ volumes, every path but the frame's fast one): a strip of 4 columns x 16
// hypotheses belongs to ONE wave.  stm_k_pq_v12m (second below; PX volumes, stm_set_agg_variant(800)): ONE column x 64 hypotheses per
// wave, the same walk with the sweep block of stm_k_pq_hsr; its comment says what differs.  stm_k_pq_v12r (third; PX volumes, the
// frame's fast path): one column per wave again, the windows summed exactly by vector adds, no MFMA.  In stm_k_pq_v12q nothing is shared:
//  * a row of the strip is 64 floats = ONE vector register, laid out exactly as the B operand of v_mfma_f32_16x16x1_4B_f32
//    wants it (lane 16 b + n = column b, hypothesis n).  The CU's register file (512 KB) is three times its LDS: the 88 input
//    rows a tile's sweep can touch and the 100 first-pass rows the second pass needs are two rings of registers per wave;
//  * no LDS, no barrier: a wave walks down its strip, per tile of 16 rows one first-pass sweep (ring 1 -> accumulators), a
//    16-instruction transposition of the accumulators into row registers (v_permlane32_swap / 16_swap), and one second-pass
//    sweep three tiles behind (ring 2 -> accumulators -> HBM);
//  * the B operand of an MFMA is addressed through the VGPR INDEX MODE (s_set_gpr_idx_on, src1 relative: measured to apply to
//    v_mfma on gfx950, tools/gpridx_probe.hip), so a sweep is ONE sequence of 22 quad blocks for every ring position;
//  * a sweep contains NO branch.  What a sweep costs is the length of the wave's own instruction stream: its MFMAs form one
//    dependent chain, issue is in order, and only what sits BETWEEN two MFMAs hides behind them.  A never-taken branch per
//    quad costs 5-14 cycles per MFMA, selects / scalar work / waits bunched between quads are added to the chain
//    (tools/quad_probe.hip: 38.6 cycles per MFMA for the block below against 53 with guards, waits and selects between the
//    quads; the compiler-scheduled C++ version of this kernel ran at 61).  So a sweep of n quads ENTERS the sequence at block
//    22 - n with one computed jump and runs to its end; a block is
//        s_set_gpr_idx_idx | MFMA | [odd block: wait for the other mask set] 4 selects for the NEXT block | MFMA |
//        [odd block: reload the set that became free, two batches ahead] | ring index += 4 (three scalar instructions) | MFMA | MFMA
//    and every block has the same size (92 bytes), so the entry point is base + 92 p + 12 (the first MFMA of a sweep is issued
//    by the prologue with the constant 0 as accumulator input: nothing is cleared);
//  * input rows arrive by buffer_load_dword in landing registers TWO steps ahead (32 rows = 8 KB in flight per wave, 64 KB per
//    CU: with one step ahead the waves spent 19 % of their time waiting for them) and are moved into the ring with the index
//    mode's relative destination.
// The whole walk is one asm block with its own register allocation (the compiler cannot be made to produce the block above:
// it merges, hoists and re-orders around guards, and re-materialises accumulators at merge points).
// Masks: the window table of stm_k_vwin_table in its static layout (one 64-bit lane mask per tile and window row, at the
// row's position inside the tile's range), read in batches of two quads (s_load_dwordx16) a batch ahead.
// Results are bit-identical to stm_k_pq_v12t (same chains, same order).  Limits: usd <= 36 (sweep range of 88 rows); longer
// arms run stm_k_pq_v12t.
#include "stm_hwin.h"

namespace stm {

constexpr int VR_TOP = 36; // a tile's sweep range starts this many rows above the tile: rows [16 u - 36, 16 u + 52)
constexpr int VR_NQ = 22;  // quads of rows in that range

// Register map of the asm block.
//   v[0:87]    ring 1: input row y in register y mod 88 (rows [16 u - 36, 16 u + 52) are live during step u)
//   v[88:103], v[228:243] landing registers of the 16 rows loaded during an even / odd step (rows [16 u + 68, 16 u + 84): two
//              steps ahead of their move into the ring -- 8 KB in flight per wave, 64 KB per CU)
//   v[104:203] ring 2: first-pass row y in register 104 + y mod 100 (the second pass of tile u - 3 reads [16 u - 84, 16 u + 4))
//   v[204:219] accumulators;  v[220:223], v[224:227] the A operands (1.0 / 0.0 per lane) of the even / odd blocks
//   v[244:245] store addresses (the store tuples are the A registers)
//   s[16:19] / s[20:23] buffer descriptors (input strip, output strip); s24 u (step), s25 / s26 ring index of row 16 u + 36 in
//   ring 1 / of row 16 u in ring 2, s27 last step + 1, s29 ring size of the running sweep, s30 ring index of the running block,
//   s[36:51] / s[52:67] mask sets of the even / odd batches, s[68:75] masks of a sweep's first quad, s[76:77] mask address of
//   block 0, s[78:79] jump target, s80 entry block, s81..s84 this step's headers (q0, n of either pass), s[86:89] the next
//   step's, s90.. temporaries, s94..s99 sweep parameters (q0, n, ring index of the range start, -, mask base), s28 u - 3
//   (s32..s35 are left alone: the ABI's stack registers).
// EXP: timing experiments (libstm_hip_timing.so only; results NOT valid): 1 = no sweeps, 2 = no loads / stores, 4 = sweeps without
// their mask waits and loads, 8 = no transposition / ring moves.  The product library instantiates EXP = 0 only.
template <int EXP>
__global__ __launch_bounds__(64, 2) void stm_k_pq_v12q(PQViews pv, const uint32_t *__restrict__ wtab, int rec, int H, int G, int NC, int nviews)
{
    // block (one wave) -> (view, group, chunk); the NC chunk waves of a strip read the same window records: consecutive blocks
    // Consecutive blocks go to different XCDs (8, each with its own L2), but the NC chunk waves of a strip read the same window
    // records: the work items are dealt out so that a strip's chunks follow each other on ONE XCD
    int wi = blockIdx.x;
    {
        const int per_xcd = gridDim.x >> 3;
        if (wi < 8 * per_xcd) wi = (wi & 7) * per_xcd + (wi >> 3);
    }
    const int c = wi % NC, sidx = wi / NC;
    if (sidx >= G * nviews) return;
    const int g = sidx % G, view = sidx / G;
    const int l = threadIdx.x;
    const int nT = (H + 15) >> 4;
    const int rsb = G * 256; // bytes between consecutive rows of the strip
    const size_t strip = ((size_t)c * H * G + g) * 64; // float index of (chunk c, row 0, group g, hypothesis 0)
    const float *in = (const float *)(view ? pv.b[1] : pv.b[0]) + strip;
    float *out = (float *)(view ? pv.a[1] : pv.a[0]) + strip;
    const uint32_t range = (uint32_t)(H - 1) * (uint32_t)rsb + 256u; // bytes of a strip up to the end of its last row
    const uint32_t *trow = wtab + ((size_t)view * nT * G + g) * rec; // record of tile 0; tile u at + u * G * rec dwords
    const int tstep = G * rec * 4;
    const int voff = (l & 15) * 16 + (l >> 4) * 4;           // lane 16 b + n loads column b of hypothesis n: float4 n, element b
    const int vst = 4 * (l >> 4) * rsb + (l & 15) * 16;      // lane 16 q + n stores row 4 q (+ i) of hypothesis n
    asm volatile(R"ASM(
        .set VR_EXP, %[exp]
        ; ---------------------------------------------------------------- macros
        ; one block of a sweep.  p = block index, rb = first register of the ring, acur / anxt = first A register this block
        ; uses / prepares, cur / nxt = first SGPR of the mask set of this block's batch / of the other set
        .macro VR_BLOCK p, rb, acur, anxt, cur, nxt
        s_set_gpr_idx_idx s30
        v_mfma_f32_16x16x1_4b_f32 v[204:219], v[\acur], v[\rb], v[204:219]
        .if (\p) & 1
        .if (VR_EXP & 4) == 0
        s_waitcnt lgkmcnt(0)
        .else
        s_nop 0
        .endif
        v_cndmask_b32_e64 v[\anxt], 0, 1.0, s[\nxt:\nxt+1]
        v_cndmask_b32_e64 v[\anxt+1], 0, 1.0, s[\nxt+2:\nxt+3]
        v_cndmask_b32_e64 v[\anxt+2], 0, 1.0, s[\nxt+4:\nxt+5]
        v_cndmask_b32_e64 v[\anxt+3], 0, 1.0, s[\nxt+6:\nxt+7]
        .else
        v_cndmask_b32_e64 v[\anxt], 0, 1.0, s[\cur+8:\cur+9]
        v_cndmask_b32_e64 v[\anxt+1], 0, 1.0, s[\cur+10:\cur+11]
        v_cndmask_b32_e64 v[\anxt+2], 0, 1.0, s[\cur+12:\cur+13]
        v_cndmask_b32_e64 v[\anxt+3], 0, 1.0, s[\cur+14:\cur+15]
        .endif
        v_mfma_f32_16x16x1_4b_f32 v[204:219], v[\acur+1], v[\rb+1], v[204:219]
        .if (\p) & 1
        .if ((\p) <= 17) && ((VR_EXP & 4) == 0)
        s_load_dwordx16 s[\cur:\cur+15], s[76:77], 64*((\p)/2+2)
        .else
        s_nop 0
        s_nop 0
        .endif
        .endif
        s_add_u32 s30, s30, 4
        s_cmp_eq_u32 s30, s29
        s_cselect_b32 s30, 0, s30
        v_mfma_f32_16x16x1_4b_f32 v[204:219], v[\acur+2], v[\rb+2], v[204:219]
        v_mfma_f32_16x16x1_4b_f32 v[204:219], v[\acur+3], v[\rb+3], v[204:219]
        .if ((\p) & 1) == 0
        s_nop 0
        s_nop 0
        s_nop 0
        .endif
        .endm
        ; a pair of blocks = batch b: even block (A operands v220.., prepares v224..), odd block (the reverse)
        .macro VR_PAIR b, rb
        .if (\b) & 1
        VR_BLOCK 2*(\b), \rb, 220, 224, 52, 36
        VR_BLOCK 2*(\b)+1, \rb, 224, 220, 52, 36
        .else
        VR_BLOCK 2*(\b), \rb, 220, 224, 36, 52
        VR_BLOCK 2*(\b)+1, \rb, 224, 220, 36, 52
        .endif
        .endm
        ; the loads a sweep starts from.  in: s94 = q0 (first quad of the sweep inside the tile's range), s95 = n (quads, >= 1),
        ; s96 = ring index of the range's first row, s29 = ring size, s[98:99] = masks of range quad 0.
        ; out: s80 = entry block 22 - n, s30 = ring index of the sweep's first row, s[76:77] = mask address of block 0;
        ; in flight: the even batch of {b0, b0 + 1} -> s[36:51], the odd one -> s[52:67] (b0 = batch of the entry block), the
        ; first quad's own masks -> s[68:75]
        .macro VR_SWEEP_ISSUE
        s_min_u32 s95, s95, 22                ; (the table cannot hold more: the jump below must stay inside the sequence)
        s_sub_u32 s80, 22, s95
        s_lshl_b32 s31, s94, 2
        s_add_u32 s30, s96, s31
        s_sub_u32 s31, s30, s29
        s_cmp_ge_u32 s30, s29
        s_cselect_b32 s30, s31, s30
        s_sub_i32 s31, s94, s80
        s_lshl_b32 s31, s31, 5
        s_ashr_i32 s97, s31, 31
        s_add_u32 s76, s98, s31
        s_addc_u32 s77, s99, s97
        s_lshr_b32 s31, s80, 1
        s_add_u32 s97, s31, 1
        s_and_b32 s97, s97, -2
        s_lshl_b32 s97, s97, 6
        s_load_dwordx16 s[36:51], s[76:77], s97
        s_or_b32 s97, s31, 1
        s_lshl_b32 s97, s97, 6
        s_load_dwordx16 s[52:67], s[76:77], s97
        s_lshl_b32 s97, s80, 5
        s_load_dwordx8 s[68:75], s[76:77], s97
        .endm
        ; the sweep: prologue (first A operands, first MFMA with the constant 0 as accumulator input), computed jump into the
        ; sequence of blocks, epilogue (the accumulators are read by vector instructions next: the last MFMA must have left
        ; the pipe)
        .macro VR_SWEEP_RUN rb
        s_waitcnt lgkmcnt(0)
        v_cndmask_b32_e64 v220, 0, 1.0, s[68:69]
        v_cndmask_b32_e64 v221, 0, 1.0, s[70:71]
        v_cndmask_b32_e64 v222, 0, 1.0, s[72:73]
        v_cndmask_b32_e64 v223, 0, 1.0, s[74:75]
        v_cndmask_b32_e64 v224, 0, 1.0, s[68:69]
        v_cndmask_b32_e64 v225, 0, 1.0, s[70:71]
        v_cndmask_b32_e64 v226, 0, 1.0, s[72:73]
        v_cndmask_b32_e64 v227, 0, 1.0, s[74:75]
        s_set_gpr_idx_on s30, 0x2
        s_mul_i32 s31, s80, 92
        s_getpc_b64 s[78:79]
VR_pc_%=_\@:
        s_add_u32 s31, s31, VR_blk0_%=_\@-VR_pc_%=_\@+12
        s_add_u32 s78, s78, s31
        s_addc_u32 s79, s79, 0
        v_mfma_f32_16x16x1_4b_f32 v[204:219], v220, v[\rb], 0
        s_setpc_b64 s[78:79]
VR_blk0_%=_\@:
        VR_PAIR 0, \rb
        VR_PAIR 1, \rb
        VR_PAIR 2, \rb
        VR_PAIR 3, \rb
        VR_PAIR 4, \rb
        VR_PAIR 5, \rb
        VR_PAIR 6, \rb
        VR_PAIR 7, \rb
        VR_PAIR 8, \rb
        VR_PAIR 9, \rb
        VR_PAIR 10, \rb
VR_end_%=_\@:
        .if (VR_end_%=_\@-VR_blk0_%=_\@) != 22*92
        .error "sweep blocks are not 92 bytes each"
        .endif
        s_set_gpr_idx_off
        s_nop 15
        s_nop 3
        .endm
        .macro VR_ZERO_ACC
        v_mov_b32 v204, 0
        v_mov_b32 v205, 0
        v_mov_b32 v206, 0
        v_mov_b32 v207, 0
        v_mov_b32 v208, 0
        v_mov_b32 v209, 0
        v_mov_b32 v210, 0
        v_mov_b32 v211, 0
        v_mov_b32 v212, 0
        v_mov_b32 v213, 0
        v_mov_b32 v214, 0
        v_mov_b32 v215, 0
        v_mov_b32 v216, 0
        v_mov_b32 v217, 0
        v_mov_b32 v218, 0
        v_mov_b32 v219, 0
        .endm
        ; four registers src.. -> ring registers rb + index.. (relative destination), then index += 4 with wrap at `size` (s31)
        .macro VR_PUT4 rb, src
        v_mov_b32 v[\rb], v[\src]
        v_mov_b32 v[\rb+1], v[\src+1]
        v_mov_b32 v[\rb+2], v[\src+2]
        v_mov_b32 v[\rb+3], v[\src+3]
        s_add_u32 s92, s92, 4
        s_cmp_eq_u32 s92, s31
        s_cselect_b32 s92, 0, s92
        s_set_gpr_idx_idx s92
        .endm
        .macro VR_LOAD_ROW lb, k
        s_cmp_lt_u32 s90, %[H]
        s_cselect_b32 s18, %[range], 0
        s_mul_i32 s91, s90, %[rsb]
        .if (VR_EXP & 2) == 0
        buffer_load_dword v[\lb+\k], %[voff], s[16:19], s91 offen nt
        .endif
        s_add_u32 s90, s90, 1
        .endm
        ; (the store tuples are the A registers, free between two sweeps; a tuple is rewritten eight instructions after its store)
        .macro VR_LOAD_FAST lb, k
        .if (VR_EXP & 2) == 0
        buffer_load_dword v[\lb+\k], %[voff], s[16:19], s91 offen nt
        .endif
        s_add_u32 s91, s91, %[rsb]
        .endm
        .macro VR_STORE_ROWS i
        v_mov_b32 v[220+4*((\i)&1)], v[204+\i]
        v_mov_b32 v[221+4*((\i)&1)], v[208+\i]
        v_mov_b32 v[222+4*((\i)&1)], v[212+\i]
        v_mov_b32 v[223+4*((\i)&1)], v[216+\i]
        v_add_u32 v[244+((\i)&1)], s85, %[vst]
        s_add_u32 s85, s85, %[rsb]
        s_nop 0
        .if (VR_EXP & 2) == 0
        buffer_store_dwordx4 v[220+4*((\i)&1):223+4*((\i)&1)], v[244+((\i)&1)], s[20:23], 0 offen nt
        .endif
        .endm

        ; ---------------------------------------------------------------- setup
        s_mov_b64 s[16:17], %[in]
        s_and_b32 s17, s17, 0xffff
        s_mov_b32 s18, 0
        s_mov_b32 s19, 0x20000
        s_mov_b64 s[20:21], %[out]
        s_and_b32 s21, s21, 0xffff
        s_mov_b32 s22, 0
        s_mov_b32 s23, 0x20000
        s_mov_b32 s24, -5                     ; u: five steps that only bring rows [0, 52) into ring 1
        s_mov_b32 s25, 44                     ; ring-1 index of row 16 u + 36 = -44
        s_mov_b32 s26, 20                     ; ring-2 index of row 16 u = -80
        s_add_u32 s27, %[nT], 3               ; the second pass runs three tiles behind
        s_mov_b64 s[86:87], 0
        s_mov_b64 s[88:89], 0
        s_mov_b32 s81, 0                      ; the first step has no tiles
        s_mov_b32 s82, 0
        s_mov_b32 s83, 0
        s_mov_b32 s84, 0
        s_sub_i32 s28, s24, 3
        .macro VR_STEP lb
        ; s81..s84 = (q0, n) of this step's first-pass tile u and second-pass tile u - 3, s28 = u - 3: set at the end of the step
        ; before, where the first masks of this step's first pass were requested too
        ; ------------------------------------------------------------ the rows loaded during the last step -> ring 1
        s_cmp_lt_i32 s24, -3
        s_cbranch_scc1 VR_nocopy_%=_\@
        .if (VR_EXP & 2) == 0
        s_waitcnt vmcnt(24)                   ; the 16 loads of the step before the last (issued since: 4 + 16 + 4 stores and loads)
        .endif
        .if (VR_EXP & 8) == 0
        s_mov_b32 s92, s25
        s_movk_i32 s31, 88
        s_set_gpr_idx_on s92, 0x8
        VR_PUT4 0, \lb
        VR_PUT4 0, \lb+4
        VR_PUT4 0, \lb+8
        VR_PUT4 0, \lb+12
        s_set_gpr_idx_off
        .endif
VR_nocopy_%=_\@:
        s_cmp_lt_i32 s24, 0
        s_cbranch_scc1 VR_loads_%=_\@
        ; ------------------------------------------------------------ first pass of tile u
        s_cmp_eq_u32 s82, 0
        s_cbranch_scc1 VR_zero1_%=_\@
        VR_SWEEP_RUN 0
        s_branch VR_p1done_%=_\@
VR_zero1_%=_\@:
        VR_ZERO_ACC
VR_p1done_%=_\@:
        ; first masks of the second pass (they travel during the transposition)
        s_cmp_eq_u32 s84, 0
        s_cbranch_scc1 VR_noissue2_%=_\@
        s_mov_b32 s94, s83
        s_mov_b32 s95, s84
        s_add_u32 s96, s26, 16                ; row 16 u - 84, and -84 = 16 (mod 100)
        s_sub_u32 s31, s96, 100
        s_cmp_ge_u32 s96, 100
        s_cselect_b32 s96, s31, s96
        s_movk_i32 s29, 100
        s_mul_i32 s92, s28, %[tstep]
        s_add_u32 s92, s92, 32
        s_add_u32 s98, %[trow_lo], s92
        s_addc_u32 s99, %[trow_hi], 0
        VR_SWEEP_ISSUE
VR_noissue2_%=_\@:
        ; accumulators (register 4 b + i of lane 16 q + n = [row 4 q + i][column b][hypothesis n]) -> row registers (register
        ; 4 q + i of lane 16 b + n): for each i a 4 x 4 transposition of (register b, lane group q)
        .if (VR_EXP & 8) == 0
        v_permlane32_swap_b32 v204, v212
        v_permlane32_swap_b32 v208, v216
        v_permlane32_swap_b32 v205, v213
        v_permlane32_swap_b32 v209, v217
        v_permlane32_swap_b32 v206, v214
        v_permlane32_swap_b32 v210, v218
        v_permlane32_swap_b32 v207, v215
        v_permlane32_swap_b32 v211, v219
        s_nop 1
        v_permlane16_swap_b32 v204, v208
        v_permlane16_swap_b32 v212, v216
        v_permlane16_swap_b32 v205, v209
        v_permlane16_swap_b32 v213, v217
        v_permlane16_swap_b32 v206, v210
        v_permlane16_swap_b32 v214, v218
        v_permlane16_swap_b32 v207, v211
        v_permlane16_swap_b32 v215, v219
        s_nop 1
        ; rows [16 u, 16 u + 16) of the first pass -> ring 2
        s_mov_b32 s92, s26
        s_movk_i32 s31, 100
        s_set_gpr_idx_on s92, 0x8
        VR_PUT4 104, 204
        VR_PUT4 104, 208
        VR_PUT4 104, 212
        VR_PUT4 104, 216
        s_set_gpr_idx_off
        .endif
VR_loads_%=_\@:
        ; ------------------------------------------------------------ rows [16 u + 68, 16 u + 84) -> the landing registers just emptied
        ; (rows above or below the image read zeros from an empty buffer; the row offset is scalar, and whether or not the
        ; range check sees it, a row of the image passes)
        s_lshl_b32 s90, s24, 4
        s_add_i32 s90, s90, 68
        s_add_i32 s91, s90, 15
        s_cmp_lt_u32 s91, %[H]                ; (unsigned: also false for rows above the image)
        s_cbranch_scc0 VR_slowloads_%=_\@
        s_cmp_lt_u32 s90, %[H]
        s_cbranch_scc0 VR_slowloads_%=_\@
        ; all sixteen rows inside the image (every step but the first and the last few): one scalar add per row
        s_mov_b32 s18, %[range]
        s_mul_i32 s91, s90, %[rsb]
        VR_LOAD_FAST \lb, 0
        VR_LOAD_FAST \lb, 1
        VR_LOAD_FAST \lb, 2
        VR_LOAD_FAST \lb, 3
        VR_LOAD_FAST \lb, 4
        VR_LOAD_FAST \lb, 5
        VR_LOAD_FAST \lb, 6
        VR_LOAD_FAST \lb, 7
        VR_LOAD_FAST \lb, 8
        VR_LOAD_FAST \lb, 9
        VR_LOAD_FAST \lb, 10
        VR_LOAD_FAST \lb, 11
        VR_LOAD_FAST \lb, 12
        VR_LOAD_FAST \lb, 13
        VR_LOAD_FAST \lb, 14
        VR_LOAD_FAST \lb, 15
        s_branch VR_loaded_%=_\@
VR_slowloads_%=_\@:
        VR_LOAD_ROW \lb, 0
        VR_LOAD_ROW \lb, 1
        VR_LOAD_ROW \lb, 2
        VR_LOAD_ROW \lb, 3
        VR_LOAD_ROW \lb, 4
        VR_LOAD_ROW \lb, 5
        VR_LOAD_ROW \lb, 6
        VR_LOAD_ROW \lb, 7
        VR_LOAD_ROW \lb, 8
        VR_LOAD_ROW \lb, 9
        VR_LOAD_ROW \lb, 10
        VR_LOAD_ROW \lb, 11
        VR_LOAD_ROW \lb, 12
        VR_LOAD_ROW \lb, 13
        VR_LOAD_ROW \lb, 14
        VR_LOAD_ROW \lb, 15
VR_loaded_%=_\@:
        s_cmp_lt_i32 s24, 0
        s_cbranch_scc1 VR_end_of_step_%=_\@
        ; ------------------------------------------------------------ second pass of tile u - 3
        s_cmp_eq_u32 s84, 0
        s_cbranch_scc1 VR_zero2_%=_\@
        VR_SWEEP_RUN 104
        s_branch VR_end_of_step_%=_\@
VR_zero2_%=_\@:
        VR_ZERO_ACC
VR_end_of_step_%=_\@:
        ; registers 4b..4b+3 of lane 16q + n = out[rows 16 v + 4q .. + 3][column b][hypothesis n]: one float4 (four columns) per
        ; row.  Always four stores (a step's loads are counted against them); before tile 0 into an empty buffer
        s_cmp_ge_i32 s28, 0
        s_cselect_b32 s22, %[range], 0
        s_lshl_b32 s85, s28, 4
        s_mul_i32 s85, s85, %[rsb]
        ; ------------------------------------------------------------ the next step: ring indices, tiles, first masks -- in front of
        ; the stores, so that the masks travel behind them and behind the next step's row moves
        s_add_u32 s25, s25, 16
        s_sub_u32 s31, s25, 88
        s_cmp_ge_u32 s25, 88
        s_cselect_b32 s25, s31, s25
        s_add_u32 s26, s26, 16
        s_sub_u32 s31, s26, 100
        s_cmp_ge_u32 s26, 100
        s_cselect_b32 s26, s31, s26
        s_add_i32 s24, s24, 1
        s_waitcnt lgkmcnt(0)                  ; the headers of its tiles, requested a step ago
        s_mov_b32 s81, s86
        s_cmp_ge_i32 s24, 0
        s_cselect_b32 s82, s87, 0
        s_cmp_lt_i32 s24, %[nT]
        s_cselect_b32 s82, s82, 0             ; first-pass tiles past the image: no window rows (their rows are zeros)
        s_sub_i32 s28, s24, 3
        s_mov_b32 s83, s88
        s_cmp_ge_i32 s28, 0
        s_cselect_b32 s84, s89, 0
        .if VR_EXP & 1
        s_mov_b32 s82, 0
        s_mov_b32 s84, 0
        .endif
        ; headers of the tiles of the step after it (tile indices clamped into the table; unused entries are masked above)
        s_sub_u32 s93, %[nT], 1
        s_add_i32 s92, s24, 1
        s_max_i32 s92, s92, 0
        s_min_i32 s92, s92, s93
        s_mul_i32 s92, s92, %[tstep]
        s_load_dwordx2 s[86:87], %[trow], s92
        s_sub_i32 s92, s24, 2
        s_max_i32 s92, s92, 0
        s_min_i32 s92, s92, s93
        s_mul_i32 s92, s92, %[tstep]
        s_load_dwordx2 s[88:89], %[trow], s92
        s_cmp_eq_u32 s82, 0
        s_cbranch_scc1 VR_noissue1_%=_\@
        s_mov_b32 s94, s81
        s_mov_b32 s95, s82
        s_add_u32 s96, s25, 16                ; row 16 u - 36 = row 16 u + 36 - 72, and -72 = 16 (mod 88)
        s_sub_u32 s31, s96, 88
        s_cmp_ge_u32 s96, 88
        s_cselect_b32 s96, s31, s96
        s_movk_i32 s29, 88
        s_mul_i32 s92, s24, %[tstep]
        s_add_u32 s92, s92, 32
        s_add_u32 s98, %[trow_lo], s92
        s_addc_u32 s99, %[trow_hi], 0
        VR_SWEEP_ISSUE
VR_noissue1_%=_\@:
        VR_STORE_ROWS 0
        VR_STORE_ROWS 1
        VR_STORE_ROWS 2
        VR_STORE_ROWS 3
        .endm
VR_loop_%=:
        VR_STEP 88
        s_cmp_ge_i32 s24, s27
        s_cbranch_scc1 VR_done_%=
        VR_STEP 228
        s_cmp_lt_i32 s24, s27
        s_cbranch_scc1 VR_loop_%=
VR_done_%=:
        s_waitcnt vmcnt(0) lgkmcnt(0)         ; the last rows and headers: nothing may be in flight when the wave ends
        .purgem VR_BLOCK
        .purgem VR_PAIR
        .purgem VR_SWEEP_ISSUE
        .purgem VR_SWEEP_RUN
        .purgem VR_ZERO_ACC
        .purgem VR_PUT4
        .purgem VR_LOAD_ROW
        .purgem VR_LOAD_FAST
        .purgem VR_STORE_ROWS
        .purgem VR_STEP
        )ASM"
                 :
                 : [in] "s"(in), [out] "s"(out), [trow] "s"(trow), [trow_lo] "s"((uint32_t)(uintptr_t)trow), [trow_hi] "s"((uint32_t)((uintptr_t)trow >> 32)),
                   [tstep] "s"(tstep), [rsb] "s"(rsb), [H] "s"(H), [nT] "s"(nT), [range] "s"(range), [voff] "v"(voff), [vst] "v"(vst), [exp] "n"(EXP)
                 : "memory", "scc", "vcc",
                   "s16", "s17", "s18", "s19", "s20", "s21", "s22", "s23", "s24", "s25", "s26", "s27", "s29", "s30", "s31", "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70", "s71", "s72", "s73", "s74", "s75", "s76", "s77", "s78", "s79", "s80", "s81", "s82", "s83", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "s96", "s97", "s98", "s99", "s28",
                   "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19",
                   "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39",
                   "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59",
                   "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79",
                   "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99",
                   "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116",
                   "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133",
                   "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143", "v144", "v145", "v146", "v147", "v148", "v149", "v150",
                   "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167",
                   "v168", "v169", "v170", "v171", "v172", "v173", "v174", "v175", "v176", "v177", "v178", "v179", "v180", "v181", "v182", "v183", "v184",
                   "v185", "v186", "v187", "v188", "v189", "v190", "v191", "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201",
                   "v202", "v203", "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218",
                   "v219", "v220", "v221", "v222", "v223", "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", "v232", "v233", "v234", "v235",
                   "v236", "v237", "v238", "v239", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247");
}

// ------------------------------------------------------------------ one column per wave, masked MFMA sweeps (PX volumes; variant 800)
// The kernel above spends one v_cndmask per MFMA: with a tile of 16 rows x 4 columns every MFMA carries 64 distinct mask bits.
// Here a wave owns ONE column and all 64 hypotheses of it (the volumes are pixel-major, PX: float index ((y 4G + x) 64 + d), a
// row of the column = 256 contiguous bytes = one register, lane 16 b + n = chunk b, hypothesis n).  The MFMA's four blocks are the
// four chunks, which share their masks, so one A register (lanes 16 a + m = window row a of a quad, tile row m) serves the
// quad's four MFMAs through CBSZ / ABID -- the sweep block of stm_k_pq_hsr (56 bytes, one select per four MFMAs), and the sweep of
// a single column is shorter than that of four (its range is the union over 16 windows instead of 64).  Chains, their order
// and every rounding are those of stm_k_pq_v12q: results are bit-identical.
// Window table: vcol_build's records (stm_hwin.h; HR_REC dwords per tile of 16 rows and column: first quad of the sweep inside the
// tile's range, quads n, the mask of the quad that sweep block p handles at 8 + 2 p, the sweep being blocks 22 - n .. 21); the 24
// mask pairs of a sweep are three s_load_dwordx16, issued where the kernel above issued its first batches.
// Rings, landing registers, the two-steps-ahead loads, the 16-row step and the three-tile lag are the kernel's above.  Register
// map: v[0:87] ring 1, v[88:103] / v[228:243] landing registers, v[104:203] ring 2, v[204:219] accumulators, v220 / v221 the A
// operand of the even / odd blocks.  s[16:19] / s[20:23] buffer descriptors (input column, output column), s24 u (step), s25 / s26
// ring index of row 16 u + 36 in ring 1 / of row 16 u in ring 2, s27 last step + 1, s28 u - 3, s29 ring size of the running
// sweep, s30 ring index of the running block, s31 temporary, s[36:83] the 24 mask pairs of the sweep, s[84:85] record address,
// then jump target, s[86:87] temporaries, s88 .. s91 this step's headers (q0, n of either pass), s[92:95] the next step's (in
// flight during a step), s96 / s97 temporaries, s98 store offset, s99 entry block (s32 .. s35 are left alone: the ABI's stack
// registers).  v[224:227] the store addresses, v[244:247] / v[248:251] the store tuples (X4).
// The first pass's accumulators are transposed into row registers for ring 2; the second pass's leave from the accumulator
// registers (register 4 b + i of lane 16 q + n = row 4 q + i, float 16 b + n of the row's record), four v_add for their row offsets:
// as sixteen dword stores of four 64-byte pieces each, float for float (X4 false), or as four 16-byte stores of four whole
// records each, float 16 b + n at float 4 n + b (X4 true, below).  Transposing them, for stores of 256 contiguous bytes with scalar
// row offsets, measured 0.013 ms slower than the dword stores (0.525 against 0.512 ms, profiles/vcol_store_forms.json).
// EXP: timing experiments (libstm_hip_timing.so only; results NOT valid): 1 = no sweeps, 2 = no loads / stores, 4 = no mask loads,
// 8 = no transposition / ring moves.
// Blocks are dealt to the XCDs as they come: neighbouring columns share no cache line of the volumes and no table record, so
// the remap of the kernel above (a strip's chunk waves on one XCD) has nothing left to keep together.
// X4: the second pass's rows leave as four buffer_store_dwordx4 (a lane's floats 16 b + n, b = 0 .. 3, of row 4 q + i to bytes
// 16 n .. 16 n + 15 of that row's record: float 16 b + n of the input record is float 4 n + b of the output record) instead of sixteen
// dword stores.  The MFMA leaves block b in registers 4 b .. 4 b + 3, so each store's tuple (i, 4 + i, 8 + i, 12 + i) is copied into
// v[244:247] / v[248:251] first: sixteen v_mov per step.  A step is then 16 loads + 4 stores.
template <int EXP, bool X4>
__global__ __launch_bounds__(64, 2) void stm_k_pq_v12m(PQViews pv, const uint32_t *__restrict__ wtab, int H, int G4, int nviews)
{
    // block (one wave) -> (view, column); columns in [W, 4G) have empty windows and write zeros
    const int x = blockIdx.x % G4, view = blockIdx.x / G4;
    if (view >= nviews) return;
    const int l = threadIdx.x;
    const int nT = (H + 15) >> 4;
    const int rsb = G4 * 256; // bytes between consecutive rows of the column
    const float *in = (const float *)(view ? pv.b[1] : pv.b[0]) + (size_t)x * 64;
    float *out = (float *)(view ? pv.a[1] : pv.a[0]) + (size_t)x * 64;
    const uint32_t range = (uint32_t)(H - 1) * (uint32_t)rsb + 256u; // bytes of a column up to the end of its last row
    const uint32_t *trow = wtab + ((size_t)view * nT * G4 + x) * HR_REC; // record of tile 0; tile u at + u * G4 * HR_REC dwords
    const int tstep = G4 * HR_REC * 4;
    const int voff = 4 * l; // lane 16 b + n = hypothesis 16 b + n
    const int vst = 4 * (l >> 4) * rsb + (l & 15) * (X4 ? 16 : 4); // lane 16 q + n stores rows 4 q (+ i) of floats (16 b +) n
    asm volatile(R"ASM(
        .set VC_EXP, %[exp]
        .set VC_X4, %[x4]
        ; ---------------------------------------------------------------- macros
        ; one block of a sweep: four MFMAs on one quad of ring rows, the A operand (lanes 16 a + m = row a of the quad, tile row m)
        ; shared through CBSZ / ABID.  p = block index, rb = first register of the ring, acur / anxt = the A registers of this / the
        ; next block
        .macro VC_BLOCK p, rb, acur, anxt
        s_set_gpr_idx_idx s30
        v_mfma_f32_16x16x1_4b_f32 v[204:219], v[\acur], v[\rb], v[204:219] cbsz:2 abid:0
        v_cndmask_b32_e64 v[\anxt], 0, 1.0, s[36+2*((\p)+1):37+2*((\p)+1)]
        v_mfma_f32_16x16x1_4b_f32 v[204:219], v[\acur], v[\rb+1], v[204:219] cbsz:2 abid:1
        s_add_u32 s30, s30, 4
        s_cmp_eq_u32 s30, s29
        s_cselect_b32 s30, 0, s30
        v_mfma_f32_16x16x1_4b_f32 v[204:219], v[\acur], v[\rb+2], v[204:219] cbsz:2 abid:2
        v_mfma_f32_16x16x1_4b_f32 v[204:219], v[\acur], v[\rb+3], v[204:219] cbsz:2 abid:3
        .endm
        .macro VC_PAIR b, rb
        VC_BLOCK 2*(\b), \rb, 220, 221
        VC_BLOCK 2*(\b)+1, \rb, 221, 220
        .endm
        ; the loads a sweep starts from.  q0 / n = the tile's header (n in 1 .. 22), s96 = ring index of the range's first row,
        ; s29 = ring size, s[84:85] = the tile's record.  out: s99 = entry block 22 - n, s30 = ring index of the sweep's first row;
        ; in flight: the 24 mask pairs (block p reads pair p + 1 for its successor, the entry block's own comes through M0)
        .macro VC_SWEEP_ISSUE q0, n
        s_sub_u32 s99, 22, \n
        s_lshl_b32 s31, \q0, 2
        s_add_u32 s30, s96, s31
        s_sub_u32 s31, s30, s29
        s_cmp_ge_u32 s30, s29
        s_cselect_b32 s30, s31, s30
        .if (VC_EXP & 4) == 0
        s_load_dwordx16 s[36:51], s[84:85], 0x20
        s_load_dwordx16 s[52:67], s[84:85], 0x60
        s_load_dwordx16 s[68:83], s[84:85], 0xa0
        .endif
        .endm
        ; the sweep: prologue (the entry block's A operand, first MFMA with the constant 0 as accumulator input), computed jump into
        ; the sequence of blocks, epilogue (the accumulators are read by vector instructions next: the last MFMA must have left
        ; the pipe)
        .macro VC_SWEEP_RUN rb
        s_waitcnt lgkmcnt(0)
        s_lshl_b32 m0, s99, 1
        s_nop 0
        s_movrels_b64 s[86:87], s[36:37]      ; the entry block's mask
        v_cndmask_b32_e64 v220, 0, 1.0, s[86:87]
        v_cndmask_b32_e64 v221, 0, 1.0, s[86:87]
        s_set_gpr_idx_on s30, 0x2
        s_mul_i32 s31, s99, 56
        s_getpc_b64 s[84:85]
VC_pc_%=_\@:
        s_add_u32 s31, s31, VC_blk0_%=_\@-VC_pc_%=_\@+12
        s_add_u32 s84, s84, s31
        s_addc_u32 s85, s85, 0
        v_mfma_f32_16x16x1_4b_f32 v[204:219], v220, v[\rb], 0 cbsz:2 abid:0
        s_setpc_b64 s[84:85]
VC_blk0_%=_\@:
        VC_PAIR 0, \rb
        VC_PAIR 1, \rb
        VC_PAIR 2, \rb
        VC_PAIR 3, \rb
        VC_PAIR 4, \rb
        VC_PAIR 5, \rb
        VC_PAIR 6, \rb
        VC_PAIR 7, \rb
        VC_PAIR 8, \rb
        VC_PAIR 9, \rb
        VC_PAIR 10, \rb
VC_end_%=_\@:
        .if (VC_end_%=_\@-VC_blk0_%=_\@) != 22*56
        .error "sweep blocks are not 56 bytes each"
        .endif
        s_set_gpr_idx_off
        s_nop 15
        s_nop 3
        .endm
        .macro VC_ZERO_ACC
        v_mov_b32 v204, 0
        v_mov_b32 v205, 0
        v_mov_b32 v206, 0
        v_mov_b32 v207, 0
        v_mov_b32 v208, 0
        v_mov_b32 v209, 0
        v_mov_b32 v210, 0
        v_mov_b32 v211, 0
        v_mov_b32 v212, 0
        v_mov_b32 v213, 0
        v_mov_b32 v214, 0
        v_mov_b32 v215, 0
        v_mov_b32 v216, 0
        v_mov_b32 v217, 0
        v_mov_b32 v218, 0
        v_mov_b32 v219, 0
        .endm
        ; accumulators (register 4 b + i of lane 16 q + n = [row 4 q + i][chunk b][hypothesis n]) -> row registers (register
        ; 4 q + i of lane 16 b + n): for each i a 4 x 4 transposition of (register b, lane group q)
        .macro VC_TRANSPOSE
        v_permlane32_swap_b32 v204, v212
        v_permlane32_swap_b32 v208, v216
        v_permlane32_swap_b32 v205, v213
        v_permlane32_swap_b32 v209, v217
        v_permlane32_swap_b32 v206, v214
        v_permlane32_swap_b32 v210, v218
        v_permlane32_swap_b32 v207, v215
        v_permlane32_swap_b32 v211, v219
        s_nop 1
        v_permlane16_swap_b32 v204, v208
        v_permlane16_swap_b32 v212, v216
        v_permlane16_swap_b32 v205, v209
        v_permlane16_swap_b32 v213, v217
        v_permlane16_swap_b32 v206, v210
        v_permlane16_swap_b32 v214, v218
        v_permlane16_swap_b32 v207, v211
        v_permlane16_swap_b32 v215, v219
        s_nop 1
        .endm
        ; four registers src.. -> ring registers rb + index.. (relative destination), then index += 4 with wrap at `size` (s31)
        .macro VC_PUT4 rb, src
        v_mov_b32 v[\rb], v[\src]
        v_mov_b32 v[\rb+1], v[\src+1]
        v_mov_b32 v[\rb+2], v[\src+2]
        v_mov_b32 v[\rb+3], v[\src+3]
        s_add_u32 s97, s97, 4
        s_cmp_eq_u32 s97, s31
        s_cselect_b32 s97, 0, s97
        s_set_gpr_idx_idx s97
        .endm
        ; rows are addressed by a scalar offset, which the buffer's range check does not see: a row outside the image goes to an
        ; empty buffer (loads return zeros, stores are dropped), a row of the image passes (its lane offset is below 256)
        .macro VC_LOAD_ROW lb, k
        s_cmp_lt_u32 s86, %[H]
        s_cselect_b32 s18, %[range], 0
        s_mul_i32 s87, s86, %[rsb]
        .if (VC_EXP & 2) == 0
        buffer_load_dword v[\lb+\k], %[voff], s[16:19], s87 offen nt
        .endif
        s_add_u32 s86, s86, 1
        .endm
        .macro VC_LOAD_FAST lb, k
        .if (VC_EXP & 2) == 0
        buffer_load_dword v[\lb+\k], %[voff], s[16:19], s87 offen nt
        .endif
        s_add_u32 s87, s87, %[rsb]
        .endm

        ; ---------------------------------------------------------------- setup
        s_mov_b64 s[16:17], %[in]
        s_and_b32 s17, s17, 0xffff
        s_mov_b32 s18, 0
        s_mov_b32 s19, 0x20000
        s_mov_b64 s[20:21], %[out]
        s_and_b32 s21, s21, 0xffff
        s_mov_b32 s22, 0
        s_mov_b32 s23, 0x20000
        s_mov_b32 s24, -5                     ; u: five steps that only bring rows [0, 52) into ring 1
        s_mov_b32 s25, 44                     ; ring-1 index of row 16 u + 36 = -44
        s_mov_b32 s26, 20                     ; ring-2 index of row 16 u = -80
        s_add_u32 s27, %[nT], 3               ; the second pass runs three tiles behind
        s_mov_b64 s[92:93], 0
        s_mov_b64 s[94:95], 0
        s_mov_b32 s88, 0                      ; the first step has no tiles
        s_mov_b32 s89, 0
        s_mov_b32 s90, 0
        s_mov_b32 s91, 0
        s_sub_i32 s28, s24, 3
        .macro VC_STEP lb
        ; s88 .. s91 = (q0, n) of this step's first-pass tile u and second-pass tile u - 3, s28 = u - 3: set at the end of the step
        ; before, where the masks of this step's first pass were requested too
        ; ------------------------------------------------------------ the rows loaded during the last step -> ring 1
        s_cmp_lt_i32 s24, -3
        s_cbranch_scc1 VC_nocopy_%=_\@
        .if (VC_EXP & 2) == 0
        .if VC_X4
        s_waitcnt vmcnt(24)                   ; the 16 loads of the step before the last (issued since: 4 stores, 16 loads, 4 stores)
        .else
        s_waitcnt vmcnt(48)                   ; the 16 loads of the step before the last (issued since: 16 stores, 16 loads, 16 stores)
        .endif
        .endif
        .if (VC_EXP & 8) == 0
        s_mov_b32 s97, s25
        s_movk_i32 s31, 88
        s_set_gpr_idx_on s97, 0x8
        VC_PUT4 0, \lb
        VC_PUT4 0, \lb+4
        VC_PUT4 0, \lb+8
        VC_PUT4 0, \lb+12
        s_set_gpr_idx_off
        .endif
VC_nocopy_%=_\@:
        s_cmp_lt_i32 s24, 0
        s_cbranch_scc1 VC_loads_%=_\@
        ; ------------------------------------------------------------ first pass of tile u
        s_cmp_eq_u32 s89, 0
        s_cbranch_scc1 VC_zero1_%=_\@
        VC_SWEEP_RUN 0
        s_branch VC_p1done_%=_\@
VC_zero1_%=_\@:
        VC_ZERO_ACC
VC_p1done_%=_\@:
        ; masks of the second pass (they travel during the transposition and the loads)
        s_cmp_eq_u32 s91, 0
        s_cbranch_scc1 VC_noissue2_%=_\@
        s_add_u32 s96, s26, 16                ; row 16 u - 84, and -84 = 16 (mod 100)
        s_sub_u32 s31, s96, 100
        s_cmp_ge_u32 s96, 100
        s_cselect_b32 s96, s31, s96
        s_movk_i32 s29, 100
        s_mul_i32 s97, s28, %[tstep]
        s_add_u32 s84, %[trow_lo], s97
        s_addc_u32 s85, %[trow_hi], 0
        VC_SWEEP_ISSUE s90, s91
VC_noissue2_%=_\@:
        .if (VC_EXP & 8) == 0
        VC_TRANSPOSE
        ; rows [16 u, 16 u + 16) of the first pass -> ring 2
        s_mov_b32 s97, s26
        s_movk_i32 s31, 100
        s_set_gpr_idx_on s97, 0x8
        VC_PUT4 104, 204
        VC_PUT4 104, 208
        VC_PUT4 104, 212
        VC_PUT4 104, 216
        s_set_gpr_idx_off
        .endif
VC_loads_%=_\@:
        ; ------------------------------------------------------------ rows [16 u + 68, 16 u + 84) -> the landing registers just emptied
        s_lshl_b32 s86, s24, 4
        s_add_i32 s86, s86, 68
        s_add_i32 s87, s86, 15
        s_cmp_lt_u32 s87, %[H]                ; (unsigned: also false for rows above the image)
        s_cbranch_scc0 VC_slowloads_%=_\@
        s_cmp_lt_u32 s86, %[H]
        s_cbranch_scc0 VC_slowloads_%=_\@
        ; all sixteen rows inside the image (every step but the first and the last few): one scalar add per row
        s_mov_b32 s18, %[range]
        s_mul_i32 s87, s86, %[rsb]
        VC_LOAD_FAST \lb, 0
        VC_LOAD_FAST \lb, 1
        VC_LOAD_FAST \lb, 2
        VC_LOAD_FAST \lb, 3
        VC_LOAD_FAST \lb, 4
        VC_LOAD_FAST \lb, 5
        VC_LOAD_FAST \lb, 6
        VC_LOAD_FAST \lb, 7
        VC_LOAD_FAST \lb, 8
        VC_LOAD_FAST \lb, 9
        VC_LOAD_FAST \lb, 10
        VC_LOAD_FAST \lb, 11
        VC_LOAD_FAST \lb, 12
        VC_LOAD_FAST \lb, 13
        VC_LOAD_FAST \lb, 14
        VC_LOAD_FAST \lb, 15
        s_branch VC_loaded_%=_\@
VC_slowloads_%=_\@:
        VC_LOAD_ROW \lb, 0
        VC_LOAD_ROW \lb, 1
        VC_LOAD_ROW \lb, 2
        VC_LOAD_ROW \lb, 3
        VC_LOAD_ROW \lb, 4
        VC_LOAD_ROW \lb, 5
        VC_LOAD_ROW \lb, 6
        VC_LOAD_ROW \lb, 7
        VC_LOAD_ROW \lb, 8
        VC_LOAD_ROW \lb, 9
        VC_LOAD_ROW \lb, 10
        VC_LOAD_ROW \lb, 11
        VC_LOAD_ROW \lb, 12
        VC_LOAD_ROW \lb, 13
        VC_LOAD_ROW \lb, 14
        VC_LOAD_ROW \lb, 15
VC_loaded_%=_\@:
        s_cmp_lt_i32 s24, 0
        s_cbranch_scc1 VC_end_of_step_%=_\@
        ; ------------------------------------------------------------ second pass of tile u - 3
        s_cmp_eq_u32 s91, 0
        s_cbranch_scc1 VC_zero2_%=_\@
        VC_SWEEP_RUN 104
        s_branch VC_end_of_step_%=_\@
VC_zero2_%=_\@:
        VC_ZERO_ACC
VC_end_of_step_%=_\@:
        ; the tile's accumulators leave below, behind the next step's bookkeeping.  Always sixteen stores (a step's loads are
        ; counted against them); before tile 0 into an empty buffer
        s_lshl_b32 s86, s28, 4                ; first row of the tile (s86 stays untouched until the stores)
        s_mul_i32 s98, s86, %[rsb]
        ; ------------------------------------------------------------ the next step: ring indices, tiles, masks -- in front of the
        ; stores, so that the masks travel behind them and behind the next step's row moves
        s_add_u32 s25, s25, 16
        s_sub_u32 s31, s25, 88
        s_cmp_ge_u32 s25, 88
        s_cselect_b32 s25, s31, s25
        s_add_u32 s26, s26, 16
        s_sub_u32 s31, s26, 100
        s_cmp_ge_u32 s26, 100
        s_cselect_b32 s26, s31, s26
        s_add_i32 s24, s24, 1
        s_waitcnt lgkmcnt(0)                  ; the headers of its tiles, requested a step ago
        s_mov_b32 s88, s92
        s_cmp_ge_i32 s24, 0
        s_cselect_b32 s89, s93, 0
        s_cmp_lt_i32 s24, %[nT]
        s_cselect_b32 s89, s89, 0             ; first-pass tiles past the image: no window rows (their rows are zeros)
        s_min_u32 s89, s89, 22                ; (the table cannot hold more: the jump must stay inside the sequence)
        s_sub_i32 s28, s24, 3
        s_mov_b32 s90, s94
        s_cmp_ge_i32 s28, 0
        s_cselect_b32 s91, s95, 0
        s_min_u32 s91, s91, 22
        .if VC_EXP & 1
        s_mov_b32 s89, 0
        s_mov_b32 s91, 0
        .endif
        ; headers of the tiles of the step after it (tile indices clamped into the table; unused entries are masked above)
        s_sub_u32 s96, %[nT], 1
        s_add_i32 s97, s24, 1
        s_max_i32 s97, s97, 0
        s_min_i32 s97, s97, s96
        s_mul_i32 s97, s97, %[tstep]
        s_load_dwordx2 s[92:93], %[trow], s97
        s_sub_i32 s97, s24, 2
        s_max_i32 s97, s97, 0
        s_min_i32 s97, s97, s96
        s_mul_i32 s97, s97, %[tstep]
        s_load_dwordx2 s[94:95], %[trow], s97
        s_cmp_eq_u32 s89, 0
        s_cbranch_scc1 VC_noissue1_%=_\@
        s_add_u32 s96, s25, 16                ; row 16 u - 36 = row 16 u + 36 - 72, and -72 = 16 (mod 88)
        s_sub_u32 s31, s96, 88
        s_cmp_ge_u32 s96, 88
        s_cselect_b32 s96, s31, s96
        s_movk_i32 s29, 88
        s_mul_i32 s97, s24, %[tstep]
        s_add_u32 s84, %[trow_lo], s97
        s_addc_u32 s85, %[trow_hi], 0
        VC_SWEEP_ISSUE s88, s89
VC_noissue1_%=_\@:
        ; straight from the accumulators: register 4 b + i of lane 16 q + n = row 4 q + i, hypothesis 16 b + n.  The whole row
        ; offset is in the vector register, so the range check sees it (rows past the image are dropped); before tile 0: empty buffer
        s_cmp_ge_i32 s86, 0
        s_cselect_b32 s22, %[range], 0
        v_add_u32 v224, s98, %[vst]
        s_add_u32 s98, s98, %[rsb]
        v_add_u32 v225, s98, %[vst]
        s_add_u32 s98, s98, %[rsb]
        v_add_u32 v226, s98, %[vst]
        s_add_u32 s98, s98, %[rsb]
        v_add_u32 v227, s98, %[vst]
        .if VC_X4
        ; the tuples of rows i = 0 .. 3, two register sets in turn (a set is rewritten five instructions after its store)
        v_mov_b32 v244, v204
        v_mov_b32 v245, v208
        v_mov_b32 v246, v212
        v_mov_b32 v247, v216
        .if (VC_EXP & 2) == 0
        buffer_store_dwordx4 v[244:247], v224, s[20:23], 0 offen nt
        .endif
        v_mov_b32 v248, v205
        v_mov_b32 v249, v209
        v_mov_b32 v250, v213
        v_mov_b32 v251, v217
        .if (VC_EXP & 2) == 0
        buffer_store_dwordx4 v[248:251], v225, s[20:23], 0 offen nt
        .endif
        v_mov_b32 v244, v206
        v_mov_b32 v245, v210
        v_mov_b32 v246, v214
        v_mov_b32 v247, v218
        .if (VC_EXP & 2) == 0
        buffer_store_dwordx4 v[244:247], v226, s[20:23], 0 offen nt
        .endif
        v_mov_b32 v248, v207
        v_mov_b32 v249, v211
        v_mov_b32 v250, v215
        v_mov_b32 v251, v219
        .if (VC_EXP & 2) == 0
        buffer_store_dwordx4 v[248:251], v227, s[20:23], 0 offen nt
        .endif
        .elseif (VC_EXP & 2) == 0
        buffer_store_dword v204, v224, s[20:23], 0 offen nt
        buffer_store_dword v208, v224, s[20:23], 0 offen offset:64 nt
        buffer_store_dword v212, v224, s[20:23], 0 offen offset:128 nt
        buffer_store_dword v216, v224, s[20:23], 0 offen offset:192 nt
        buffer_store_dword v205, v225, s[20:23], 0 offen nt
        buffer_store_dword v209, v225, s[20:23], 0 offen offset:64 nt
        buffer_store_dword v213, v225, s[20:23], 0 offen offset:128 nt
        buffer_store_dword v217, v225, s[20:23], 0 offen offset:192 nt
        buffer_store_dword v206, v226, s[20:23], 0 offen nt
        buffer_store_dword v210, v226, s[20:23], 0 offen offset:64 nt
        buffer_store_dword v214, v226, s[20:23], 0 offen offset:128 nt
        buffer_store_dword v218, v226, s[20:23], 0 offen offset:192 nt
        buffer_store_dword v207, v227, s[20:23], 0 offen nt
        buffer_store_dword v211, v227, s[20:23], 0 offen offset:64 nt
        buffer_store_dword v215, v227, s[20:23], 0 offen offset:128 nt
        buffer_store_dword v219, v227, s[20:23], 0 offen offset:192 nt
        .endif
        .endm
VC_loop_%=:
        VC_STEP 88
        s_cmp_ge_i32 s24, s27
        s_cbranch_scc1 VC_done_%=
        VC_STEP 228
        s_cmp_lt_i32 s24, s27
        s_cbranch_scc1 VC_loop_%=
VC_done_%=:
        s_waitcnt vmcnt(0) lgkmcnt(0)         ; the last rows, masks and headers: nothing may be in flight when the wave ends
        .purgem VC_BLOCK
        .purgem VC_PAIR
        .purgem VC_SWEEP_ISSUE
        .purgem VC_SWEEP_RUN
        .purgem VC_ZERO_ACC
        .purgem VC_TRANSPOSE
        .purgem VC_PUT4
        .purgem VC_LOAD_ROW
        .purgem VC_LOAD_FAST
        .purgem VC_STEP
        )ASM"
                 :
                 : [in] "s"(in), [out] "s"(out), [trow] "s"(trow), [trow_lo] "s"((uint32_t)(uintptr_t)trow), [trow_hi] "s"((uint32_t)((uintptr_t)trow >> 32)),
                   [tstep] "s"(tstep), [rsb] "s"(rsb), [H] "s"(H), [nT] "s"(nT), [range] "s"(range), [voff] "v"(voff), [vst] "v"(vst), [exp] "n"(EXP), [x4] "n"(X4 ? 1 : 0)
                 : "memory", "scc", "vcc",
                   "s16", "s17", "s18", "s19", "s20", "s21", "s22", "s23", "s24", "s25", "s26", "s27", "s28", "s29", "s30", "s31", "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70", "s71", "s72", "s73", "s74", "s75", "s76", "s77", "s78", "s79", "s80", "s81", "s82", "s83", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "s96", "s97", "s98", "s99",
                   "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19",
                   "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39",
                   "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59",
                   "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79",
                   "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99",
                   "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116",
                   "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133",
                   "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143", "v144", "v145", "v146", "v147", "v148", "v149", "v150",
                   "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167",
                   "v168", "v169", "v170", "v171", "v172", "v173", "v174", "v175", "v176", "v177", "v178", "v179", "v180", "v181", "v182", "v183", "v184",
                   "v185", "v186", "v187", "v188", "v189", "v190", "v191", "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201",
                   "v202", "v203", "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218",
                   "v219", "v220", "v221", "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", "v232", "v233", "v234", "v235",
                   "v236", "v237", "v238", "v239", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251");
}

// ------------------------------------------------------------------ one column per wave, exact windows as runs of vector adds
// The default of the frame's fast path.  stm_k_pq_v12m above sweeps, per tile of 16 rows, the union of the tile's windows with
// masked MFMAs: half of its add slots multiply by zero.  With one column per wave and lane = hypothesis the
// window [y - armU, y + armD) is the same for all 64 lanes, so its sum is a straight run of `v_add_f32 acc, row, acc` over exactly
// its rows, in the reference's order (d_ca_cross_sum.cu:148-198): no mask, no select, no accumulator tile, no transposition.
// Every register of a run is NAMED: through the VGPR index mode an add issues in 4 cycles instead of 2
// (tools/vadd_chain_probe.hip), so each ring has one sequence of 72 adds per slot a window can end in (72 sequences of 292 bytes,
// 42 KB for both rings), a window is one computed jump into the sequence of its last row, 72 - L adds from the start, and a window
// that crosses the ring's end is summed like any other.  The jump offset of every row comes ready from the table (stm_hwin.h,
// va_entry: one dword per row, 9 MB at 1080p where the masks took 67 MB).
// A step handles one row: the second pass of row y - 36 (ring 2 -> acc -> HBM), the first pass of row y (ring 1 -> acc), then acc
// enters ring 2 and input row y + 36 ring 1, both at slot y mod 72 (relative destination: the index mode is on for these two moves
// only).  Input rows arrive in sixteen landing registers, sixteen steps ahead of their move (4 KB in flight per wave).  Every step
// issues exactly one load and one store, so that one vmcnt value fits all steps: rows below the image are read as the last row
// (no window reaches them), stores of rows outside the image go to an empty buffer.
// Register map: v0 accumulator, v[1:72] ring 1, v[73:144] ring 2, v[145:160] landing registers.  s[16:19] / s[20:23] buffer
// descriptors (input column, output column), s24 y, s25 y mod 72, s26 byte offset of the next row to load, s27 that of the last
// row, s28 byte offset of row y - 36, s29 table offset of row y, s30 y - 36, s[36:37] / s[38:39] the sequences of ring 1 / ring 2,
// s[40:41] / s[42:43] table of the column at row -36 / -72, s[44:45] / s[46:47] entries (first, second pass) of an even / odd
// step, s[48:49] jump target, s[50:51] return address, s52 last step + 1, s31 y - first row of the first pass (s32 .. s35 are left alone: the ABI's stack registers).
// Blocks: the kernel's 163 registers let three waves share a SIMD, V12R_SLOTS on the chip.  `full` columns (a multiple of the slots)
// are one block each; every column beyond them is cut into `parts` row ranges, one block each, which start when the whole columns
// end -- 3840 columns as 3840 blocks left 768 of them running alone on their SIMDs at the end, a third of the kernel's time.  A
// range [y0, y1) begins 72 rows early with the ring's fill and ends 36 rows late (the first pass of the rows its last windows need).
// s53 / s54: 36 + y0 and y1 - y0 (the second pass's rows), s55 / s56: first row and number of the first pass's rows, s57 / s58: the
// steps [y0 + 36, min(y1 + 36, H)) at which both passes have a row of the block: sixteen such steps in a row run without asking.
// Results are bit-identical to stm_k_pq_v12m (the same chains in the same order; adding 0.0 * row changed nothing).
// X4: lane 16 b + n stores at float 4 n + b of the record (order 2 of stm_px_order), else at float 16 b + n.
// EXP: timing experiments (libstm_hip_timing.so only; results NOT valid): 1 = no sums, 2 = no loads / stores.
constexpr int V12R_SLOTS = 3 * 4 * 256; // resident waves of the chip: three on each SIMD of MI355X's 256 CUs
template <int EXP, bool X4>
__global__ __launch_bounds__(64) void stm_k_pq_v12r(PQViews pv, const uint32_t *__restrict__ atab, int H, int G4, int nviews, int full, int parts)
{
    // block (one wave) -> (view, column, rows [y0, y1)); columns in [W, 4G) have empty windows and write zeros
    const int b = blockIdx.x, cidx = b < full ? b : full + (b - full) / parts, part = b < full ? 0 : (b - full) % parts, np = b < full ? 1 : parts;
    const int x = cidx % G4, view = cidx / G4;
    if (view >= nviews) return;
    const int y0 = (int)((long long)H * part / np), y1 = (int)((long long)H * (part + 1) / np);
    const int ys = max(y0 - 108, -36);                              // first step: row ys + 36 is the first to enter ring 1
    const int p1lo = max(y0 - 36, 0), p1n = min(y1 + 36, H) - p1lo; // rows of the first pass
    const int l = threadIdx.x;
    const int rsb = G4 * 256; // bytes between consecutive rows of the column
    const float *in = (const float *)(view ? pv.b[1] : pv.b[0]) + (size_t)x * 64;
    float *out = (float *)(view ? pv.a[1] : pv.a[0]) + (size_t)x * 64;
    const uint32_t last = (uint32_t)(H - 1) * (uint32_t)rsb, range = last + 256u; // bytes of a column up to the end of its last row
    const uint32_t *tcol = atab + ((size_t)view * G4 + x) * va_rows(H);           // the column's entries, row -VA_PAD first
    const int voff = 4 * l;                                                       // lane 16 b + n = float 16 b + n of a record
    const int vst = X4 ? 4 * (4 * (l & 15) + (l >> 4)) : 4 * l;
    static_assert(VA_RING == 72 && VA_LAG == 36 && VA_SEQ == 292 && VA_PAD == 72, "the asm block below is written for these");
    asm volatile(R"ASM(
        .set VA_EXP, %[exp]
        .macro VA_FILL k
        .if (VA_EXP & 2) == 0
        buffer_store_dword v0, %[vst], s[20:23], 0 offen nt   ; (empty buffer: counted, not written)
        buffer_load_dword v[145+\k], %[voff], s[16:19], s26 offen nt
        .endif
        s_add_u32 s26, s26, %[rsb]
        s_min_u32 s26, s26, s27
        .endm
        ; one row.  k = step mod 16 (the landing register), cur / nxt = first SGPR of this / the next step's entries, g = 1: either
        ; pass asks whether its row is one of the block's (the steps at both ends of a range), g = 0: both are (seven scalar
        ; instructions less)
        .macro VA_STEP k, cur, nxt, g
        s_waitcnt lgkmcnt(0)                  ; this step's entries, requested a step ago
        s_add_u32 s29, s29, 4
        s_load_dword s[\nxt], s[40:41], s29
        s_load_dword s[\nxt+1], s[42:43], s29
        ; ------------------------------------------------------------ second pass of row y - 36
        .if \g
        s_sub_u32 s30, s24, s53
        s_cmp_lt_u32 s30, s54                 ; (unsigned: also false above the range)
        s_cselect_b32 s22, %[range], 0
        s_cbranch_scc0 VA_skip2_%=_\@
        .endif
        v_mov_b32 v0, 0
        .if (VA_EXP & 1) == 0
        s_add_u32 s48, s38, s[\cur+1]
        s_addc_u32 s49, s39, 0
        s_swappc_b64 s[50:51], s[48:49]
        .endif
VA_skip2_%=_\@:
        .if (VA_EXP & 2) == 0
        buffer_store_dword v0, %[vst], s[20:23], s28 offen nt
        .endif
        s_add_u32 s28, s28, %[rsb]
        ; ------------------------------------------------------------ first pass of row y
        .if \g
        s_sub_u32 s31, s24, s55
        s_cmp_lt_u32 s31, s56
        s_cbranch_scc0 VA_skip1_%=_\@
        .endif
        v_mov_b32 v0, 0
        .if (VA_EXP & 1) == 0
        s_add_u32 s48, s36, s[\cur]
        s_addc_u32 s49, s37, 0
        s_swappc_b64 s[50:51], s[48:49]
        .endif
VA_skip1_%=_\@:
        .if (VA_EXP & 2) == 0
        s_waitcnt vmcnt(31)                   ; the load of sixteen steps ago (issued since: 15 loads, 16 stores)
        .endif
        s_set_gpr_idx_on s25, 0x8
        v_mov_b32 v73, v0                     ; first-pass row y -> ring 2
        v_mov_b32 v1, v[145+\k]               ; input row y + 36 -> ring 1
        s_set_gpr_idx_off
        .if (VA_EXP & 2) == 0
        buffer_load_dword v[145+\k], %[voff], s[16:19], s26 offen nt   ; row y + 52 (below the image: the last row again)
        .endif
        s_add_u32 s26, s26, %[rsb]
        s_min_u32 s26, s26, s27
        s_add_u32 s25, s25, 1
        s_cmp_eq_u32 s25, 72
        s_cselect_b32 s25, 0, s25
        s_add_i32 s24, s24, 1
        .endm

        ; ---------------------------------------------------------------- setup
        s_mov_b64 s[16:17], %[in]
        s_and_b32 s17, s17, 0xffff
        s_mov_b32 s18, %[range]
        s_mov_b32 s19, 0x20000
        s_mov_b64 s[20:21], %[out]
        s_and_b32 s21, s21, 0xffff
        s_mov_b32 s22, 0
        s_mov_b32 s23, 0x20000
        s_mov_b32 s24, %[ys]                  ; the first steps only bring rows into ring 1 (a column from its top: 36 steps, rows [0, 36))
        s_mov_b32 s25, %[ys72]
        s_mov_b32 s27, %[last]
        s_add_u32 s26, s24, 36
        s_mul_i32 s26, s26, %[rsb]
        s_min_u32 s26, s26, s27
        s_sub_u32 s28, s24, 36
        s_mul_i32 s28, s28, %[rsb]
        s_add_u32 s29, s24, 36
        s_lshl_b32 s29, s29, 2
        s_mov_b32 s53, %[p2lo]
        s_mov_b32 s54, %[p2n]
        s_mov_b32 s55, %[p1lo]
        s_mov_b32 s56, %[p1n]
        s_mov_b32 s57, %[mlo]
        s_mov_b32 s58, %[mhi]
        s_add_u32 s40, %[tcol_lo], 144
        s_addc_u32 s41, %[tcol_hi], 0
        s_mov_b32 s42, %[tcol_lo]
        s_mov_b32 s43, %[tcol_hi]
        s_add_u32 s52, %[y1], 36
        s_load_dword s44, s[40:41], s29
        s_load_dword s45, s[42:43], s29
        s_getpc_b64 s[36:37]
VA_pc_%=:
        s_add_u32 s36, s36, VA_seq_%=-VA_pc_%=
        s_addc_u32 s37, s37, 0
        s_add_u32 s38, s36, 72*292
        s_addc_u32 s39, s37, 0
        v_mov_b32 v0, 0
        VA_FILL 0
        VA_FILL 1
        VA_FILL 2
        VA_FILL 3
        VA_FILL 4
        VA_FILL 5
        VA_FILL 6
        VA_FILL 7
        VA_FILL 8
        VA_FILL 9
        VA_FILL 10
        VA_FILL 11
        VA_FILL 12
        VA_FILL 13
        VA_FILL 14
        VA_FILL 15
        s_branch VA_loop_%=
        ; ---------------------------------------------------------------- the sequences: ring 1 (slots e + 1 .. e + 72), then
        ; ring 2 (its slot of a row lies 36 further on)
VA_seq_%=:
        .set VA_e, 0
        .rept 72
        .set VA_j, 0
        .rept 72
        v_add_f32 v0, v[1+(VA_e+1+VA_j)%%72], v0
        .set VA_j, VA_j+1
        .endr
        s_setpc_b64 s[50:51]
        .set VA_e, VA_e+1
        .endr
        .set VA_e, 0
        .rept 72
        .set VA_j, 0
        .rept 72
        v_add_f32 v0, v[73+(VA_e+37+VA_j)%%72], v0
        .set VA_j, VA_j+1
        .endr
        s_setpc_b64 s[50:51]
        .set VA_e, VA_e+1
        .endr
VA_seqend_%=:
        .if (VA_seqend_%=-VA_seq_%=) != 144*292
        .error "a sequence is not 292 bytes"
        .endif
VA_loop_%=:
        ; sixteen steps that ask (the ends of the range) ...
        s_cmp_ge_i32 s24, s52
        s_cbranch_scc1 VA_done_%=
        VA_STEP 0, 44, 46, 1
        VA_STEP 1, 46, 44, 1
        VA_STEP 2, 44, 46, 1
        VA_STEP 3, 46, 44, 1
        VA_STEP 4, 44, 46, 1
        VA_STEP 5, 46, 44, 1
        VA_STEP 6, 44, 46, 1
        VA_STEP 7, 46, 44, 1
        VA_STEP 8, 44, 46, 1
        VA_STEP 9, 46, 44, 1
        VA_STEP 10, 44, 46, 1
        VA_STEP 11, 46, 44, 1
        VA_STEP 12, 44, 46, 1
        VA_STEP 13, 46, 44, 1
        VA_STEP 14, 44, 46, 1
        VA_STEP 15, 46, 44, 1
        s_cmp_lt_i32 s24, s57
        s_cbranch_scc1 VA_loop_%=
        s_add_u32 s30, s24, 16
        s_cmp_gt_i32 s30, s58
        s_cbranch_scc1 VA_loop_%=
        s_mov_b32 s22, %[range]
VA_main_%=:
        ; ... and sixteen that do not, while all sixteen rows belong to both passes
        VA_STEP 0, 44, 46, 0
        VA_STEP 1, 46, 44, 0
        VA_STEP 2, 44, 46, 0
        VA_STEP 3, 46, 44, 0
        VA_STEP 4, 44, 46, 0
        VA_STEP 5, 46, 44, 0
        VA_STEP 6, 44, 46, 0
        VA_STEP 7, 46, 44, 0
        VA_STEP 8, 44, 46, 0
        VA_STEP 9, 46, 44, 0
        VA_STEP 10, 44, 46, 0
        VA_STEP 11, 46, 44, 0
        VA_STEP 12, 44, 46, 0
        VA_STEP 13, 46, 44, 0
        VA_STEP 14, 44, 46, 0
        VA_STEP 15, 46, 44, 0
        s_add_u32 s30, s24, 16
        s_cmp_le_i32 s30, s58
        s_cbranch_scc1 VA_main_%=
        s_branch VA_loop_%=
VA_done_%=:
        s_waitcnt vmcnt(0) lgkmcnt(0)         ; the last rows and entries: nothing may be in flight when the wave ends
        .purgem VA_FILL
        .purgem VA_STEP
        )ASM"
                 :
                 : [in] "s"(in), [out] "s"(out), [tcol_lo] "s"((uint32_t)(uintptr_t)tcol), [tcol_hi] "s"((uint32_t)((uintptr_t)tcol >> 32)), [rsb] "s"(rsb), [y1] "s"(y1),
                   [ys] "s"(ys), [ys72] "s"((ys + 72) % 72), [p2lo] "s"(36 + y0), [p2n] "s"(y1 - y0), [p1lo] "s"(p1lo), [p1n] "s"(p1n), [mlo] "s"(y0 + 36), [mhi] "s"(min(y1 + 36, H)), [range] "s"(range), [last] "s"(last), [voff] "v"(voff), [vst] "v"(vst), [exp] "n"(EXP)
                 : "memory", "scc", "vcc",
                   "s16", "s17", "s18", "s19", "s20", "s21", "s22", "s23", "s24", "s25", "s26", "s27", "s28", "s29", "s30", "s31", "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58",
                   "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19",
                   "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37",
                   "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55",
                   "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73",
                   "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91",
                   "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108",
                   "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124",
                   "v125", "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140",
                   "v141", "v142", "v143", "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156",
                   "v157", "v158", "v159", "v160");
}

// The per-column window table of `nviews` views from the arm planes (the frame path builds it inside stm_k_cross_arms instead).
// A wave = the tile's 16 rows x four columns, lane 16 c + m.  ENTRIES: the arms as jump offsets (va_entry) for stm_k_pq_v12r, else
// the mask records (vcol_build) of stm_k_pq_v12m.
template <bool ENTRIES>
__global__ __launch_bounds__(256) void stm_k_vcol_table(PQViews v, uint32_t *__restrict__ tab, int H, int W, int G, int nT)
{
    __shared__ uint32_t ev_all[4][4 * 96];
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, g = blockIdx.x * 4 + wv, u = blockIdx.y, view = blockIdx.z;
    if (g >= G) return; // uniform per wave; no block-wide barrier below
    const u8 *__restrict__ armU = view ? v.armU[1] : v.armU[0], *__restrict__ armD = view ? v.armD[1] : v.armD[0];
    const int c = l >> 4, m = l & 15, y = u * 16 + m, x = 4 * g + c;
    int aU = 0, aD = 0; // no window outside the image
    if (y < H && x < W) {
        aU = armU[(size_t)y * W + x];
        aD = armD[(size_t)y * W + x];
    }
    if (ENTRIES) tab[((size_t)view * (4 * G) + x) * va_rows(H) + VA_PAD + y] = va_entry(y, aU, aD);
    else vcol_build(tab + (size_t)(view * nT + u) * (4 * G) * HR_REC, ev_all[wv], u, 4 * g, y - aU, aU + aD);
}

bool aggv_supports(int usd) { return usd >= 1 && usd <= VR_TOP; }
int aggv_table_top() { return VR_TOP; }
int aggv_table_rec() { return 8 + 8 * (VR_NQ + 2); } // header + 22 quads + the batch read-ahead

// both vertical passes, vol_b -> vol_a, for `nviews` views; `tab` / `rec`: the window table of stm_k_vwin_table (static layout)
void launch_pq_v12q(PQViews &v, int nviews, const uint32_t *tab, int rec, int H, int W, int G, int NC)
{
    (void)W;
    const dim3 grid(G * nviews * NC);
#ifdef STM_TIMING
    switch (timing_knobs()) {
    case 1: STM_LAUNCH(stm_k_pq_v12q<1>, grid, dim3(64), 0, stream(), v, tab, rec, H, G, NC, nviews); break;
    case 2: STM_LAUNCH(stm_k_pq_v12q<2>, grid, dim3(64), 0, stream(), v, tab, rec, H, G, NC, nviews); break;
    case 3: STM_LAUNCH(stm_k_pq_v12q<3>, grid, dim3(64), 0, stream(), v, tab, rec, H, G, NC, nviews); break;
    case 4: STM_LAUNCH(stm_k_pq_v12q<4>, grid, dim3(64), 0, stream(), v, tab, rec, H, G, NC, nviews); break;
    case 6: STM_LAUNCH(stm_k_pq_v12q<6>, grid, dim3(64), 0, stream(), v, tab, rec, H, G, NC, nviews); break;
    case 8: STM_LAUNCH(stm_k_pq_v12q<8>, grid, dim3(64), 0, stream(), v, tab, rec, H, G, NC, nviews); break;
    case 9: STM_LAUNCH(stm_k_pq_v12q<9>, grid, dim3(64), 0, stream(), v, tab, rec, H, G, NC, nviews); break;
    default: STM_LAUNCH(stm_k_pq_v12q<0>, grid, dim3(64), 0, stream(), v, tab, rec, H, G, NC, nviews); break;
    }
#else
    STM_LAUNCH(stm_k_pq_v12q<0>, grid, dim3(64), 0, stream(), v, tab, rec, H, G, NC, nviews);
#endif
    STM_CHECK_LAUNCH();
}


// 800: the masked-MFMA column kernel stm_k_pq_v12m and its mask records instead of stm_k_pq_v12r and its table of arms
bool aggv_col_vadd() { return (agg_variant() / 100) % 10 != 8; }
size_t aggv_col_table_dwords(int nviews, int H, int W)
{
    if (aggv_col_vadd()) return (size_t)nviews * (4 * cdiv(W, 4)) * va_rows(H) + 64;
    return (size_t)nviews * cdiv(H, 16) * (4 * cdiv(W, 4)) * HR_REC + 64;
}

void launch_vcol_table(PQViews &v, int nviews, uint32_t *tab, int H, int W)
{
    const int G = cdiv(W, 4), nT = cdiv(H, 16);
    if (aggv_col_vadd()) STM_LAUNCH(stm_k_vcol_table<true>, dim3(cdiv(G, 4), nT, nviews), dim3(256), 0, stream(), v, tab, H, W, G, nT);
    else STM_LAUNCH(stm_k_vcol_table<false>, dim3(cdiv(G, 4), nT, nviews), dim3(256), 0, stream(), v, tab, H, W, G, nT);
    STM_CHECK_LAUNCH();
}

// both vertical passes on PX volumes, vol_b -> vol_a, for `nviews` views; `tab`: the per-column table in the form of
// aggv_col_vadd() (the arms as jump offsets, or vcol_build's mask records under 800)
void launch_pq_v12r(PQViews &v, int nviews, const uint32_t *tab, int H, int W, int G, bool x4)
{
    (void)W;
    const int G4 = 4 * G;
    const dim3 grid(G4 * nviews);
    const bool vadd = aggv_col_vadd();
    // stm_k_pq_v12r: whole columns in rounds that fill the chip's wave slots, the rest in row ranges of 128 rows and more
    const int ncol = G4 * nviews, full = ncol / V12R_SLOTS * V12R_SLOTS, rest = ncol - full;
    const int parts = rest ? std::max(1, std::min(V12R_SLOTS / rest, H / 128)) : 1;
    const dim3 grid_a(full + rest * parts);
#define STM_V12R_LAUNCH(E)                                                                                      \
    {                                                                                                           \
        if (vadd && x4) STM_LAUNCH((stm_k_pq_v12r<E, true>), grid_a, dim3(64), 0, stream(), v, tab, H, G4, nviews, full, parts);   \
        else if (vadd) STM_LAUNCH((stm_k_pq_v12r<E, false>), grid_a, dim3(64), 0, stream(), v, tab, H, G4, nviews, full, parts);   \
        else if (x4) STM_LAUNCH((stm_k_pq_v12m<E, true>), grid, dim3(64), 0, stream(), v, tab, H, G4, nviews);      \
        else STM_LAUNCH((stm_k_pq_v12m<E, false>), grid, dim3(64), 0, stream(), v, tab, H, G4, nviews);             \
    }
#ifdef STM_TIMING
    switch (timing_knobs()) {
    case 1: STM_V12R_LAUNCH(1); break;
    case 2: STM_V12R_LAUNCH(2); break;
    case 3: STM_V12R_LAUNCH(3); break;
    case 4: STM_V12R_LAUNCH(4); break;
    case 8: STM_V12R_LAUNCH(8); break;
    default: STM_V12R_LAUNCH(0); break;
    }
#else
    STM_V12R_LAUNCH(0);
#endif
#undef STM_V12R_LAUNCH
    STM_CHECK_LAUNCH();
}

} // namespace stm
