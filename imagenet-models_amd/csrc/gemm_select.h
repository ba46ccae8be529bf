// Kernel-form selection of ga_gemm (NT) and ga_wgrad (TN): plain host C++, a pure function of the descriptor, the CU count and
// the knob values.  No HIP, no statics, no knob look-ups: gemm.hip fills Knobs, calls nt_select / tn_select and launches what
// they name; ga_gemm_form / ga_wgrad_form print it; the CPU tests pin it (tests/golden/gemm_forms.json).
//
// ga_gemm tries the forms in the order of the NtForm enum and takes the first that applies (DESIGN.md section 4 has the table).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include "../../include/gaext.h"

void ga_set_error(const char* fmt, ...);   // runtime.hip
// conv3.hip, next to the direct kernels they guard: does the kernel take this ga_gemm product / with how many workgroups (each
// with its own partial sums in the workspace) does it take this ga_wgrad product (0: it does not).  Pure, no knob inside.
bool ga_conv3_c64_eligible(const ga_gemm_desc* d);
bool ga_conv0_c8_eligible(const ga_gemm_desc* d);
int ga_conv3_c64_wgrad_wgs(const ga_wgrad_desc* d, int num_cus);
int ga_conv3s2_c64_wgrad_wgs(const ga_wgrad_desc* d, int num_cus);
int ga_conv0_c8_wgrad_wgs(const ga_wgrad_desc* d, int num_cus);
int ga_stem4_wgrad_wgs(const ga_wgrad_desc* d, int num_cus);

namespace gasel {

enum { EPI_GENERIC = -1, EPI_PLAIN = 0, EPI_FC1 = 1, EPI_FC2 = 2, EPI_DG2 = 3 };

// every knob the selection reads, at its default; the caller overwrites them from the knob table.  NT_R3, NT_PP, NT_T256, NT_DMA2:
// epilogue masks (1 plain, 2 fc1, 4 fc2, 8 dgrad2), -1 = heuristic; the predicate that reads a knob says what it does
struct Knobs {
    int NT_R3 = -1, NT_R3_NEIGH2 = 1, NT_R3_CONV3S2 = 1, NT_PP = -1, NT_PP_MINK = 512, NT_BIG = -1, NT_DMA = 1, NT_DMA2 = 10,
        NT_DMA2_MINK = 256, NT_T256 = -1;
    int TN2 = 1, TN2_PATCH2 = 1, TN2_WGS = 0, TN2_PART_MIN = 65536;
    int CONV3_DIRECT = 1, CONV0_DIRECT = 1, STEM4_WGRAD_DIRECT = 1;      // the direct kernels of conv3.hip
    int FEWROWS = 1, FEWROWS_MAXM = 512;                                 // the few-row forms of gemm_fewrows.hip (their own entry points)
};

Knobs current_knobs();      // gemm.hip: the knob table's values (the one place that looks knobs up)

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }
inline bool aligned16(const void* p) { return (addr(p) & 15) == 0; }

#define GA_SEL_REQUIRE(cond, ...) \
    do { if (!(cond)) { ga_set_error(__VA_ARGS__); return GA_ERR_BAD_ARG; } } while (0)

// ---- ga_gemm ----
inline int nt_validate(const ga_gemm_desc* d) {
    GA_SEL_REQUIRE(d && d->A && d->B && d->C, "ga_gemm: null operand");
    GA_SEL_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0 && d->batch >= 1, "ga_gemm: bad shape M=%d N=%d K=%d batch=%d", d->M,
                   d->N, d->K, d->batch);
    GA_SEL_REQUIRE(d->dtype == GA_F32 || d->dtype == GA_BF16, "ga_gemm: bad dtype %d", d->dtype);
    const int epc = d->dtype == GA_BF16 ? 8 : 4;
    GA_SEL_REQUIRE(aligned16(d->A) && aligned16(d->B) && aligned16(d->C), "ga_gemm: operands must be 16-byte aligned");
    GA_SEL_REQUIRE(d->ldb % epc == 0 && d->strideB % epc == 0, "ga_gemm: ldb/strideB must be multiples of %d", epc);
    GA_SEL_REQUIRE(d->K % epc == 0, "ga_gemm: K=%d must be a multiple of %d (pad the operand)", d->K, epc);
    if (d->a_kind == GA_A_PLAIN) {
        GA_SEL_REQUIRE(d->lda % epc == 0 && d->strideA % epc == 0, "ga_gemm: lda/strideA must be multiples of %d", epc);
    } else if (d->a_kind == GA_A_PATCH2) {
        GA_SEL_REQUIRE(d->a_C % epc == 0 && d->a_H % 2 == 0 && d->a_W % 2 == 0 && d->K == 4 * d->a_C &&
                           (long)d->M % ((d->a_H / 2) * (d->a_W / 2)) == 0,
                       "ga_gemm: PATCH2 needs C%%%d==0, even H,W, K==4C", epc);
    } else if (d->a_kind == GA_A_CONV3) {
        GA_SEL_REQUIRE(d->a_C % epc == 0 && d->K == 9 * d->a_C && (long)d->M % (d->a_H * d->a_W) == 0,
                       "ga_gemm: CONV3 needs C%%%d==0, K==9C", epc);
    } else if (d->a_kind == GA_A_CONV3S2) {
        GA_SEL_REQUIRE(d->a_C % epc == 0 && d->K == 9 * d->a_C && (long)d->M % (((d->a_H + 1) / 2) * ((d->a_W + 1) / 2)) == 0,
                       "ga_gemm: CONV3S2 needs C%%%d==0, K==9C", epc);
    } else if (d->a_kind == GA_A_NEIGH2) {
        GA_SEL_REQUIRE(d->a_C % epc == 0 && d->K == 4 * d->a_C && (long)d->M % (d->a_H * d->a_W) == 0,
                       "ga_gemm: NEIGH2 needs C%%%d==0, K==4C", epc);
    } else if (d->a_kind == GA_A_STEM4_NCHW) {
        GA_SEL_REQUIRE(d->a_C == 3 && d->K == 48 && d->a_H % 4 == 0 && d->a_W % 4 == 0, "ga_gemm: STEM4 needs C=3,K=48");
    } else {
        GA_SEL_REQUIRE(false, "ga_gemm: bad a_kind %d", d->a_kind);
    }
    if (d->c_kind == GA_C_UNPATCH2) {
        GA_SEL_REQUIRE(d->c_C % 8 == 0 && d->N == 4 * d->c_C && !d->c_f32, "ga_gemm: UNPATCH2 needs N==4*c_C, c_C%%8==0");
    } else {
        GA_SEL_REQUIRE(d->c_kind == GA_C_PLAIN, "ga_gemm: bad c_kind");
    }
    if (d->H) GA_SEL_REQUIRE(aligned16(d->H) && d->ldh % 8 == 0, "ga_gemm: H alignment");
    if (d->C2) GA_SEL_REQUIRE(aligned16(d->C2) && d->c_kind == GA_C_PLAIN && !d->c_f32 && (d->c2_mode == 1 || d->c2_mode == 2),
                              "ga_gemm: C2 needs a plain, dtype-typed C and c2_mode 1|2");
    if (d->R) GA_SEL_REQUIRE(aligned16(d->R) && d->ldr % 8 == 0, "ga_gemm: R alignment");
    if (d->rowscale) GA_SEL_REQUIRE(d->rows_per_scale > 0, "ga_gemm: rows_per_scale");
    // vector stores need an 8-element aligned leading dimension; otherwise every piece takes the scalar path,
    // which the kernel selects per piece only at the N edge -> require it here.
    GA_SEL_REQUIRE(d->c_kind != GA_C_PLAIN || d->ldc % 8 == 0, "ga_gemm: ldc=%ld must be a multiple of 8", (long)d->ldc);
    return GA_OK;
}

// the forms in the order ga_gemm tries them
enum NtForm { NT_CONV3_DIRECT, NT_CONV0_DIRECT, NT_R3G, NT_R3, NT_DMA256, NT_PP, NT_T256, NT_DMA128, NT_BIG, NT_STAGED };

// tile of 32*tnw columns (t256: 8) and 64*nwm rows; pre: the epilogue operand (R / H) is prefetched into registers
struct NtSel {
    int form, epi, tnw, nwm;
    bool pre;
};

// the compile-time epilogue that the descriptor's epilogue fields match (a hot shape of the training step), whatever the
// layouts of A and C: the ring gather serves the gather layouts, every other fused form wants plain ones (nt_select)
inline int classify_epilogue(const ga_gemm_desc* d) {
    if (d->a_act != GA_ACT_NONE || d->alpha != 1.0f || d->c_f32 || d->relu_after) return EPI_GENERIC;
    const bool act0 = d->act == GA_ACT_NONE;
    if (d->act == GA_ACT_GELU && (!d->C2 || d->c2_mode == 2) && !d->H && !d->R && !d->rowscale && !d->colsum) return EPI_FC1;
    if (act0 && !d->C2 && !d->H && d->R && !d->colsum) return EPI_FC2;
    if (act0 && !d->C2 && d->H && d->h_is_deriv && !d->R && !d->rowscale) return EPI_DG2;
    if (act0 && !d->C2 && !d->H && !d->R && !d->rowscale) return EPI_PLAIN;
    return EPI_GENERIC;
}

// the gather layouts the ring form reads / writes itself (plain epilogue only)
inline bool ring_gather_a(const ga_gemm_desc* d) {
    return d->a_kind == GA_A_PATCH2 || d->a_kind == GA_A_NEIGH2 || d->a_kind == GA_A_CONV3S2;
}

// 8-wave ping-pong form: NT_PP = bit mask of epilogues; unset: plain / fc1 / fc2, for launches whose K loop is long enough to
// carry the un-overlapped epilogue (K >= NT_PP_MINK, default 512) and whose last column tile is not mostly empty.
// Its own: lda, ldb >= 64; no offset bound on C, H, R.  (nt_validate has, for every fused form: K, lda, ldb, ldh, ldr multiples
// of 8 and 16-byte A, B, C, C2, H, R; N and, with GA_C_UNPATCH2, ldc are free there.)
inline bool pp_wanted(const ga_gemm_desc* d, int epi, int num_cus, const Knobs& k) {
    const bool e = k.NT_PP >= 0;
    const int mask = e ? k.NT_PP : 7;       // (dgrad2: its stored-GELU' operand is read inside the un-overlapped epilogue: measured slower)
    if (!mask || d->dtype != GA_BF16 || d->a_kind != GA_A_PLAIN || epi == EPI_GENERIC || !((mask >> epi) & 1)) return false;
    if (d->N % 8 != 0 || d->K < (e ? 256 : k.NT_PP_MINK) || d->ldc % 8 != 0) return false;
    if ((long)d->M * d->lda >= (1L << 30) || (long)d->N * d->ldb >= (1L << 30) || d->lda < 64 || d->ldb < 64) return false;   // 32-bit byte offsets
    const int tn = ceil_div(d->N, 256);
    if (!e && tn * 256 - d->N > tn * 256 / 8) return false;        // > 12.5 % of the column tiles' MFMA work on columns that do not exist
    return (long)ceil_div(d->M, 256) * tn * d->batch >= num_cus / 2;
}

// 3-slot ring form (256 x 128 tiles, two workgroups per CU): NT_R3 = bit mask of epilogues; -1 = the heuristic below.
// `epi` is the epilogue it would run: EPI_PLAIN for the gather layouts.  Its own: the gather exceptions, K >= 64, offset bounds
// on every operand it reads with 32-bit offsets (A, B, C, H, R).
inline bool r3_wanted(const ga_gemm_desc* d, int epi, int num_cus, const Knobs& k) {
    const bool forced = k.NT_R3 >= 0;
    const int mask = forced ? k.NT_R3 : 15;
    const bool neigh2 = d->a_kind == GA_A_NEIGH2;       // 2 x 2 neighbourhoods (data gradient of the 3 x 3 / stride-2 convs): plain epilogue only
    const bool conv3s2 = d->a_kind == GA_A_CONV3S2;     // the 3 x 3 / stride-2 convs on even maps: plain epilogue only
    const bool patch2 = ring_gather_a(d);               // 2 x 2 / stride-2 patches (downsample convs): plain epilogue only
    if (patch2 && (epi != EPI_PLAIN || d->a_C % 16 != 0 || d->K != (conv3s2 ? 9 : 4) * d->a_C || 4L * d->M * d->a_C >= (1L << 30) ||
                   d->a_batch_mod || d->batch != 1))
        return false;
    if (neigh2 && (d->a_C % 32 != 0 || (long)d->M % ((long)d->a_H * d->a_W) != 0 || !k.NT_R3_NEIGH2)) return false;
    if (conv3s2 && (d->a_C % 32 != 0 || d->a_H % 2 != 0 || d->a_W % 2 != 0 || d->a_W < 4 ||
                    (long)d->M % ((long)(d->a_H / 2) * (d->a_W / 2)) != 0 || !k.NT_R3_CONV3S2))
        return false;
    if (!mask || d->dtype != GA_BF16 || (d->a_kind != GA_A_PLAIN && !patch2) || epi == EPI_GENERIC || !((mask >> epi) & 1)) return false;
    if (d->N % 8 != 0 || d->K < 64 || d->ldc % 8 != 0) return false;
    if ((!patch2 && (long)d->M * d->lda >= (1L << 30)) || (long)d->N * d->ldb >= (1L << 30)) return false;   // 32-bit byte offsets
    const bool unpatch2 = d->c_kind == GA_C_UNPATCH2;   // scatter of the downsample conv's data gradient: plain epilogue only
    if (unpatch2 && (epi != EPI_PLAIN || d->colsum || d->c_C % 8 != 0 || d->N != 4 * d->c_C || 4L * d->M * d->c_C >= (1L << 30) || d->batch != 1))
        return false;
    if ((!unpatch2 && (long)d->M * d->ldc >= (1L << 30)) || (d->c_kind != GA_C_PLAIN && !unpatch2) || d->c_f32) return false;
    if (epi == EPI_DG2 && (long)d->M * d->ldh >= (1L << 30)) return false;
    if (epi == EPI_FC2 && (long)d->M * d->ldr >= (1L << 30)) return false;
    if (d->bias && (addr(d->bias) & 3)) return false;
    if (forced) return true;
    // heuristic from same-process A/B rounds against the other forms (tools/r3_ab.py, gpurun_out/r03/r3_ab*.log; MI355X):
    //   fc1 / fc2 / dgrad2 epilogues at M = 6,272 .. 200,704, K = 192 .. 3072: x1.04 .. 1.76 everywhere measured
    //   plain: ahead for K <= 512 (x1.13 .. 1.18) and for the K = 768 .. 2208 launches of the heads (x1.03 .. 1.10); behind the
    //   8-wave ping-pong body on very wide / very long / very tall launches (N 2208: x0.91, K 3072: x0.83, 8192^3: x0.88,
    //   M 73,856 of the ViT trunk: x0.91 .. 0.97) and behind the 128-column forms at N < 384 with a mid-length K (x0.95)
    // gather kinds: the alternative is the register-staged gather (110-240 TFLOP/s on these launches, 0.105 ms for the 100 tiles
    // of merge3's half-batch forward against 0.03 here)
    if (neigh2 || conv3s2) return (long)ceil_div(d->M, 256) * ceil_div(d->N, 128) >= 16;
    if ((long)ceil_div(d->M, 256) * ceil_div(d->N, 128) * d->batch < num_cus / 2) return false;      // too few tiles to fill the chip
    const bool pp = pp_wanted(d, epi, num_cus, k);      // where the ping-pong form would take the launch, it is the measured rival
    if (d->M >= 65536 && pp) return false;
    if (epi != EPI_PLAIN) return true;
    if (d->K <= 512) return true;
    if (pp) return d->N < 2048 && d->K < 3072;
    return d->N >= 384 ? d->K < 3072 : d->K >= 1024;
}

// the LDS-DMA forms address their operands with 32-bit byte offsets from the matrix base; they check nothing else of the layout
// (ga_gemm's validation has: 8-element leading dimensions, 16-byte pointers)
inline bool dma_offsets_fit(const ga_gemm_desc* d) { return (long)d->M * d->lda < (1L << 30) && (long)d->N * d->ldb < (1L << 30); }
inline bool dma_operands(const ga_gemm_desc* d, int epi) {
    return d->dtype == GA_BF16 && d->a_kind == GA_A_PLAIN && epi != EPI_GENERIC && dma_offsets_fit(d);
}

// LDS-DMA form: 256-row tiles of 128 or 96 columns, plain bf16 operands, one of the compile-time epilogues
inline bool dma256_wanted(const ga_gemm_desc* d, int epi, int tnw, int num_cus, const Knobs& k) {
    const int mode = k.NT_DMA;                    // 0 off, 1 heuristic (default), 2 every eligible launch
    if (!mode || !dma_operands(d, epi) || (tnw != 4 && tnw != 3)) return false;
    if ((long)ceil_div(d->M, 256) * ceil_div(d->N, 32 * tnw) * d->batch < num_cus) return false;
    // measured (tools/gemm_bench.py): ahead only for the fc2 epilogue with a long reduction (K >= 1024, +8..20 %);
    // mode 2 forces it on every eligible launch (tests, experiments)
    return mode == 2 || (epi == EPI_FC2 && tnw == 4 && d->K >= 1024);
}

// 256 x 256 tile, 8 waves (64 x 128 each), LDS-DMA into a 2-slot ring: wide-N launches
inline bool t256_wanted(const ga_gemm_desc* d, int epi, int num_cus, const Knobs& k) {
    // unset: every epilogue, but only for the very tall launches (M >= 65536: the ViT trunk's 73,856 token rows, -4.8 % on the
    // MAP-ViT-B/384 step); on the ConvNeXt / CSWin stage-2/3 shapes (M = 50,176) the form measured -12 .. +5 % and stays off
    const int mask = k.NT_T256 >= 0 ? k.NT_T256 : ((d->M >= 65536 && d->N >= 768) ? 15 : 0);      // (N >= 768: the CSWin stem's N = 256 launches lose 2 %)
    if (!mask || !dma_operands(d, epi)) return false;
    if (d->N % 256 != 0 || d->K < 256) return false;
    if ((long)ceil_div(d->M, 256) * (d->N / 256) * d->batch < num_cus) return false;
    return (mask >> epi) & 1;
}

// 128 x 128 tile, 4 waves, LDS-DMA into a 2-slot ring, 80 KiB: two workgroups per CU without the ds_write staging pass
inline bool dma128_wanted(const ga_gemm_desc* d, int epi, int tnw, const Knobs& k) {
    // NT_DMA2 unset: fc1 and dgrad2 (stage-2 shapes, same box, after the DMA went through buffer resources: fc1 0.126 -> 0.119 ms,
    // dgrad2 0.137 -> 0.118; fc2 / dgrad1 are 3-5 % slower with it and keep the register-staged form)
    if (tnw != 4 || !k.NT_DMA2 || !dma_operands(d, epi)) return false;
    if (d->K < k.NT_DMA2_MINK) return false;
    return (k.NT_DMA2 >> epi) & 1;
}

// 256-row tiles (8 waves, one workgroup per CU) for the two epilogues that carry a prefetched epilogue operand
// (fc2: + shortcut, dgrad2: * gelu'): their 4-wave form sits at 160-170 VGPRs = 2 workgroups per CU, and the wide
// tile reads the weight slab once per 256 rows.  Measured on MI355X (tools/gemm_bench.py): dgrad2 1.35-1.45x,
// fc2 1.1-1.2x; the plain / fc1 epilogues (120 VGPRs, 4 workgroups per CU) are 5-15 % SLOWER with it.
inline bool big_wanted(const ga_gemm_desc* d, int epi, int tnw, int num_cus, const Knobs& k) {
    if (tnw != 4 || d->dtype != GA_BF16 || d->a_kind != GA_A_PLAIN || (epi != EPI_FC2 && epi != EPI_DG2)) return false;
    if (k.NT_BIG >= 0) return k.NT_BIG != 0;      // 0 / 1 override for experiments
    return (long)ceil_div(d->M, 256) * ceil_div(d->N, 128) * d->batch >= 2L * num_cus;
}

// N-tile width: 128 when it divides N, else 96 (stage-0 C = 96, concat 2208 = 23*96), else 64; ragged N -> least waste
inline int nt_tile_width(int N) {
    if (N % 128 == 0) return 4;
    if (N % 96 == 0) return 3;
    if (N % 64 == 0) return 2;
    const long w4 = (long)ceil_div(N, 128) * 128, w3 = (long)ceil_div(N, 96) * 96, w2 = (long)ceil_div(N, 64) * 64;
    return (w4 <= w3 && w4 <= w2) ? 4 : (w3 <= w2 ? 3 : 2);
}

// the form ga_gemm launches for a descriptor that passed nt_validate: the first of the tried order that applies
inline NtSel nt_select(const ga_gemm_desc* d, int num_cus, const Knobs& k) {
    const int tnw = nt_tile_width(d->N);
    if (k.CONV3_DIRECT && ga_conv3_c64_eligible(d)) return {NT_CONV3_DIRECT, EPI_PLAIN, 0, 0, false};
    if (k.CONV0_DIRECT && ga_conv0_c8_eligible(d)) return {NT_CONV0_DIRECT, EPI_PLAIN, 0, 0, false};
    const int cls = classify_epilogue(d);
    const bool plain_layout = d->a_kind == GA_A_PLAIN && d->c_kind == GA_C_PLAIN;
    // downsample conv (2 x 2 / stride 2) straight from the NHWC map / its data gradient (GA_C_UNPATCH2), the 3 x 3 / stride-2 gathers
    const bool ring_layout = !plain_layout && (d->a_kind == GA_A_PLAIN || ring_gather_a(d));
    if (ring_layout && cls == EPI_PLAIN && r3_wanted(d, EPI_PLAIN, num_cus, k))
        return {d->a_kind == GA_A_NEIGH2 || d->a_kind == GA_A_CONV3S2 ? NT_R3G : NT_R3, EPI_PLAIN, 4, 4, false};
    const int epi = plain_layout ? cls : EPI_GENERIC;      // every other fused epilogue reads and writes plain matrices
    const bool pre = epi == EPI_FC2 || epi == EPI_DG2;
    if (r3_wanted(d, epi, num_cus, k)) return {NT_R3, epi, 4, 4, false};
    if (dma256_wanted(d, epi, tnw, num_cus, k)) return {NT_DMA256, epi, tnw, 4, pre};
    if (pp_wanted(d, epi, num_cus, k)) return {NT_PP, epi, 8, 4, false};
    if (t256_wanted(d, epi, num_cus, k)) return {NT_T256, epi, 8, 4, false};     // no registers left for the prefetch
    if (dma128_wanted(d, epi, tnw, k)) return {NT_DMA128, epi, 4, 2, pre};
    if (big_wanted(d, epi, tnw, num_cus, k)) return {NT_BIG, epi, 4, 4, true};
    // register-staged 128 x (128 | 96 | 64) tiles, bf16 or fp32, any gather: the epilogue-operand prefetch exists for bf16 only
    // (32 extra VGPRs)
    const bool bf = d->dtype == GA_BF16;
    if (d->a_kind != GA_A_PLAIN) return {NT_STAGED, EPI_GENERIC, tnw, 2, false};
    return {NT_STAGED, epi, tnw, 2, bf && (pre || (epi == EPI_GENERIC && (d->H || d->R)))};
}

// stable name of a selection: r3:fc1, r3g:plain, dma256x96:plain, pp:fc2, t256:dg2, dma128:fc1, big:dg2,
// staged128:generic+pre (+gather: A is gathered; +f32: fp32 operands), conv3_direct, conv0_direct
inline void nt_form_name(const ga_gemm_desc* d, const NtSel& s, char* buf, size_t n) {
    const char* const form[] = {"conv3_direct", "conv0_direct", "r3g", "r3", "dma256x", "pp", "t256", "dma128", "big", "staged"};
    const char* const epi[] = {"generic", "plain", "fc1", "fc2", "dg2"};
    if (s.form <= NT_CONV0_DIRECT) snprintf(buf, n, "%s", form[s.form]);
    else if (s.form != NT_DMA256 && s.form != NT_STAGED) snprintf(buf, n, "%s:%s", form[s.form], epi[s.epi + 1]);
    else snprintf(buf, n, "%s%d:%s%s%s%s", form[s.form], 32 * s.tnw, epi[s.epi + 1], s.form == NT_STAGED && s.pre ? "+pre" : "",
                  d->a_kind != GA_A_PLAIN ? "+gather" : "", d->dtype == GA_F32 ? "+f32" : "");
}

// ---- ga_wgrad ----
inline int tn_validate(const ga_wgrad_desc* d) {
    GA_SEL_REQUIRE(d && d->Y && d->X && d->dW, "ga_wgrad: null operand");
    GA_SEL_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0 && d->batch >= 1 && d->split_m >= 1, "ga_wgrad: bad shape");
    GA_SEL_REQUIRE(d->dtype == GA_F32 || d->dtype == GA_BF16, "ga_wgrad: bad dtype %d", d->dtype);
    const int epc = d->dtype == GA_BF16 ? 8 : 4;
    GA_SEL_REQUIRE(aligned16(d->Y) && aligned16(d->X), "ga_wgrad: operands must be 16-byte aligned");
    GA_SEL_REQUIRE(d->N % epc == 0 && d->ldy % epc == 0 && d->strideY % epc == 0, "ga_wgrad: N/ldy must be multiples of %d",
                   epc);
    if (d->x_kind == GA_A_PLAIN) {
        // K (an OUTPUT dim here) may be ragged as long as the X rows are padded to a chunk multiple
        GA_SEL_REQUIRE(d->ldx % epc == 0 && d->strideX % epc == 0 && d->ldx >= (d->K + epc - 1) / epc * epc,
                       "ga_wgrad: ldx must be a multiple of %d and cover K rounded up", epc);
    } else if (d->x_kind == GA_A_PATCH2 || d->x_kind == GA_A_NEIGH2 || d->x_kind == GA_A_CONV3 || d->x_kind == GA_A_CONV3S2) {
        const int taps = d->x_kind == GA_A_PATCH2 || d->x_kind == GA_A_NEIGH2 ? 4 : 9;
        GA_SEL_REQUIRE(d->x_C % epc == 0 && d->K == taps * d->x_C, "ga_wgrad: %s needs K==%dC",
                       d->x_kind == GA_A_PATCH2 ? "PATCH2" : d->x_kind == GA_A_NEIGH2 ? "NEIGH2" : d->x_kind == GA_A_CONV3 ? "CONV3" : "CONV3S2", taps);
    } else if (d->x_kind == GA_A_STEM4_NCHW) {
        GA_SEL_REQUIRE(d->x_C == 3 && d->K == 48, "ga_wgrad: STEM4 needs C=3,K=48");
    } else {
        GA_SEL_REQUIRE(false, "ga_wgrad: bad x_kind %d", d->x_kind);
    }
    return GA_OK;
}

// the forms in the order ga_wgrad tries them.  The direct kernels (conv3.hip) and the partial tiles of the wide form need the
// caller's workspace: without it a direct kernel's launch goes to TN_TN, the wide form combines its row splits with atomics
enum TnForm { TN_CONV3_DIRECT, TN_CONV3S2_DIRECT, TN_CONV0_DIRECT, TN_STEM4_DIRECT, TN_TN2, TN_TN };

struct TnSel {
    int form;
    int split;         // direct kernels: workgroups, each with its own partial sums; TN_TN2: row splits; TN_TN: split_m
    size_t ws_bytes;   // what ga_wgrad_workspace reports: bytes the first applicable form wants, whether or not d has them
    bool partials;     // TN_TN2: the row splits go through partial tiles in the workspace (else fp32 atomics)
};

// the wide form needs whole 32-row stages, plain bf16 operands, and an output that is accumulated into (so that it
// may choose its own row split); it pays once the reduction is long enough to amortise the 256 x 256 tile
// GA_A_PATCH2 operands (TN2_PATCH2, default 1): NHWC map of even sides with C % 8 == 0, K == 4 C, byte offsets < 2^31
inline bool tn2_eligible(const ga_wgrad_desc* d, const Knobs& k) {
    if (!(k.TN2 && d->dtype == GA_BF16 && d->x_act == GA_ACT_NONE && d->M % 32 == 0 && d->M >= 8192 &&
          (d->accumulate || d->split_m > 1) && (long)d->M * d->ldy < (1L << 31)))                    // 32-bit byte offsets
        return false;
    if (d->x_kind == GA_A_PLAIN) return (long)d->M * d->ldx < (1L << 31);
    if (d->x_kind == GA_A_PATCH2)
        return k.TN2_PATCH2 && d->x_C > 0 && d->x_C % 8 == 0 && d->K == 4 * d->x_C && d->x_H > 0 && d->x_W > 0 &&
               d->x_H % 2 == 0 && d->x_W % 2 == 0 && d->M % ((long)(d->x_H / 2) * (d->x_W / 2)) == 0 &&
               8L * d->M * d->x_C < (1L << 31);
    return false;
}

// row split of the wide form and the bytes of partial-tile workspace it wants (0: combine with atomics)
inline size_t tn2_plan(const ga_wgrad_desc* d, int num_cus, const Knobs& k, int* split_out) {
    const int tiles = ceil_div(d->N, 256) * ceil_div(d->K, 256) * d->batch;
    const int stages = d->M / 32;
    // 3/4 of the CUs: in the train step these launches share the chip with the dgrad chain (asynchronous lane), and
    // fewer row splits mean fewer partial tiles to write and reduce (same-box A/B: 192 vs 256 workgroups -0.13 ms/step)
    const int cus = k.TN2_WGS > 0 ? k.TN2_WGS : num_cus * 3 / 4;
    int split = std::max(1, std::min(stages / 8, cus / tiles));               // one workgroup per CU
    split = ceil_div(stages, ceil_div(stages, split));                        // no empty row range
    *split_out = split;
    const long nk = (long)d->N * d->K;
    const long nk_min = k.TN2_PART_MIN;      // 256 x 256 outputs (CSWin proj) included: -0.2 ms/step there, neutral elsewhere
    return (split > 1 && nk >= nk_min) ? (size_t)d->batch * split * nk * sizeof(float) : 0;   // small outputs: atomics are cheaper
}

// the form ga_wgrad launches: the first of the tried order that applies and has its workspace
inline TnSel tn_select(const ga_wgrad_desc* d, int num_cus, const Knobs& k) {
    const bool has_ws = d->workspace != nullptr;
    int wgs;
    size_t need;
    auto direct = [&](int form, size_t per_wg) -> TnSel {
        need = (size_t)wgs * per_wg * sizeof(float);
        if (has_ws && (size_t)d->ws_bytes >= need) return {form, wgs, need, true};
        return {TN_TN, d->split_m, need, false};      // (none of the direct kernels' operands is one the wide form takes)
    };
    if (k.CONV3_DIRECT && (wgs = ga_conv3_c64_wgrad_wgs(d, num_cus))) return direct(TN_CONV3_DIRECT, 64 * 576);
    if (k.CONV3_DIRECT && (wgs = ga_conv3s2_c64_wgrad_wgs(d, num_cus))) return direct(TN_CONV3S2_DIRECT, 64 * 576);
    if (k.CONV0_DIRECT && (wgs = ga_conv0_c8_wgrad_wgs(d, num_cus))) return direct(TN_CONV0_DIRECT, 64 * 72);
    if (k.STEM4_WGRAD_DIRECT && (wgs = ga_stem4_wgrad_wgs(d, num_cus))) return direct(TN_STEM4_DIRECT, (size_t)d->N * 49);
    if (tn2_eligible(d, k)) {
        int split;
        need = tn2_plan(d, num_cus, k, &split);
        // partial tiles + one reduce launch when the caller provided the workspace ga_wgrad_workspace() asks for; fp32 atomics
        // into dW otherwise (slower for wide outputs, same result up to summation order)
        return {TN_TN2, split, need, need && has_ws && (size_t)d->ws_bytes >= need};
    }
    return {TN_TN, d->split_m, 0, false};
}

// stable name: conv3_wgrad_direct:wgs256 (also conv3s2_, conv0_, stem4_), tn2:split20:partials, tn2p:split4:atomics (tn2p:
// GA_A_PATCH2 operand), tn.  With the descriptor, the name determines ws_bytes.
inline void tn_form_name(const ga_wgrad_desc* d, const TnSel& s, char* buf, size_t n) {
    const char* const form[] = {"conv3_wgrad_direct", "conv3s2_wgrad_direct", "conv0_wgrad_direct", "stem4_wgrad_direct", "tn2", "tn"};
    if (s.form == TN_TN) snprintf(buf, n, "tn");
    else if (s.form != TN_TN2) snprintf(buf, n, "%s:wgs%d", form[s.form], s.split);
    else snprintf(buf, n, "tn2%s:split%d:%s", d->x_kind == GA_A_PATCH2 ? "p" : "", s.split, s.partials ? "partials" : "atomics");
}

// ---- the few-row forms (gemm_fewrows.hip): entry points of their own, ga_gemm_fewrows / ga_wgrad_fewrows ----
// nt_select / tn_select and their answers stay what they are (the recorded corpus pins them); these predicates say which
// descriptors the new entry points take themselves.  Everything else they forward to ga_gemm / ga_wgrad.
//
// Two conditions besides what the kernels can compute: the launch has few rows, and the form ga_gemm / ga_wgrad would choose leaves
// the chip mostly empty -- fewer of its 128-row (128 x 128) tiles, times batch (and split_m), than half the compute units.  That
// keeps the per-sample Gram products (M = 196, batch 256: 1024 tiles) and the 96 x 2316 products of the Gram embedding (batch 8: 152
// and 592 tiles) where they are.
// The row bound: same-process sweep of M = 64 .. 1024 at N x K = 192 x 768 and 768 x 192 (tools/fewrows_ab.py,
// profiles/r05_fewrows_sweep.json; MI355X, us per launch, old -> new): NT x1.7 .. 2.3 up to M = 512 (13.5 -> 6.0 at 256 x 192 x 768)
// and x1.23 at 1024 x 768 x 192 (8.4 -> 6.8, 768 workgroups); TN x1.8 .. 2.2 at every M (12.7 -> 6.0 at M = 256, 32.2 -> 15.0 at 1024).
// FEWROWS_MAXM (default 512) is the bound -- the last M at which both shapes keep x1.7 -- and a knob so that the sweep can look past it.

inline bool nt_fewrows_wanted(const ga_gemm_desc* d, int num_cus, const Knobs& k) {
    if (!k.FEWROWS || d->dtype != GA_BF16 || d->a_kind != GA_A_PLAIN || d->c_kind != GA_C_PLAIN || d->a_act != GA_ACT_NONE ||
        d->relu_after)
        return false;
    // epilogues: bias, alpha, c_f32, row scale, residual, column sums; GELU (+ GELU' into C2) only as the fc1 epilogue of the bf16
    // forms (its logistic GELU); H only as the stored derivative (dgrad2)
    if (d->act != GA_ACT_NONE ? classify_epilogue(d) != EPI_FC1 : d->C2 != nullptr) return false;
    if (d->H && !d->h_is_deriv) return false;
    if (d->colsumsq && !d->colsum) return false;
    // 8-byte accesses of 4 consecutive bf16 (16-byte of 4 floats) at every batch element
    if (d->strideC % 4 != 0 || (d->R && d->strideR % 4 != 0) || (d->H && d->strideH % 4 != 0) || (d->bias && (addr(d->bias) & 3)))
        return false;
    if (d->M > k.FEWROWS_MAXM || d->batch > 65535) return false;
    // only what ga_gemm runs on the register-staged body: a launch that a knob forces onto another form stays on that form
    if (nt_select(d, num_cus, k).form != NT_STAGED) return false;
    return (long)ceil_div(d->M, 128) * ceil_div(d->N, 32 * nt_tile_width(d->N)) * d->batch < num_cus / 2;
}

// fewrows32x32:plain | fc1 | fc2 | dg2 | generic (the epilogue class of the descriptor), or none
inline void nt_fewrows_name(const ga_gemm_desc* d, bool wanted, char* buf, size_t n) {
    const char* const epi[] = {"generic", "plain", "fc1", "fc2", "dg2"};
    if (wanted) snprintf(buf, n, "fewrows32x32:%s", epi[classify_epilogue(d) + 1]);
    else snprintf(buf, n, "none");
}

// the weight gradient with a short reduction: plain bf16 operands; an output that is stored or accumulated by its one workgroup
// (split_m > 1 without `accumulate` means atomics into a zeroed dW: the caller's row split is its own business)
inline bool tn_fewrows_wanted(const ga_wgrad_desc* d, int num_cus, const Knobs& k) {
    if (!k.FEWROWS || d->dtype != GA_BF16 || d->x_kind != GA_A_PLAIN || d->x_act != GA_ACT_NONE) return false;
    if (!d->accumulate && d->split_m > 1) return false;
    if (d->M > k.FEWROWS_MAXM || d->batch > 65535) return false;
    if (tn_select(d, num_cus, k).form != TN_TN) return false;      // (M < 8192 rules the wide form out; the direct kernels have gathers)
    return (long)ceil_div(d->N, 128) * ceil_div(d->K, 128) * d->split_m * d->batch < num_cus / 2;
}

#undef GA_SEL_REQUIRE

}  // namespace gasel
