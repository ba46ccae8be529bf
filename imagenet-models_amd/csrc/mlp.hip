// Fused MLP bodies for the narrow stages (bf16, C = 96 / 192, hidden H = 4C): the 128 x H hidden tile never goes to HBM.
//
//   ga_mlp_fwd:  Y = R + rowscale * (gelu(X W1^T + b1) W2^T + b2)                  (Block.forward, ga_convnext.py:86-101:
//                pwconv1 -> GELU -> pwconv2 -> gamma -> DropPath -> residual; LayerNorm affine and gamma are folded into
//                the effective weights by ga_weight_prep)
//   ga_mlp_bwd:  re-computes Hd = X W1^T + b1, then A = gelu(Hd), DH = (DY W2) * gelu'(Hd), DX = DH W1;
//                writes A and DH once (the weight-gradient GEMMs read them) and DX.
//
// Why: at C = 96 the unfused fc1 / fc2 / dgrad2 / dgrad1 GEMMs have 40-60 FLOP per HBM byte and run at the HBM rate
// (4.0-4.4 TB/s, 170-390 TFLOP/s); the hidden activation and its GELU' (8C per token written, 8C read back) are 3/4 of
// the forward traffic of a block.  Here a workgroup owns 128 token rows: X (and DY) stay in LDS, the hidden dimension is
// walked in chunks of HC columns, each chunk's weights come from L2 through registers (prefetched one chunk ahead),
// and the chunk of the hidden tile lives in accumulators / one LDS tile between the two chained MFMA products.
//
// LDS operand images are "k slabs": [rows][32 bf16] = 64-byte rows, the 16-byte unit c of row r at c ^ ((r >> 2) & 3),
// so the ds_read_b128 of a 16x16x32 fragment (16 rows x one unit per 16-lane group) covers all 16 slots of the 256-byte
// bank row.  The weight fragment is the MFMA's first operand: a lane then holds 4 CONSECUTIVE hidden / output columns
// of ONE token row, i.e. an 8-byte piece of the next product's row-major operand tile.
#include <stdlib.h>
#include <algorithm>
#include "common.h"

namespace {

constexpr int BM = 128;

// workgroup barrier that orders LDS traffic only: the weight pieces of the NEXT chunk stay in flight across it
// (__syncthreads() would wait for vmcnt(0) as well and expose their L2 latency once per chunk)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ unsigned slab_off(int r, int c) { return r * 64 + ((c ^ ((r >> 2) & 3)) << 4); }

__device__ __forceinline__ bf16x8_t frag(const unsigned char* slab, int r0, int lane) {
    return *reinterpret_cast<const bf16x8_t*>(slab + slab_off(r0 + (lane & 15), lane >> 4));
}

// global rows [row0, row0 + ROWS) x (32 * KS) bf16 -> KS slabs of [ROWS][64 B]; rows >= limit are zero.  All the loads of a
// thread are issued before the first LDS write (one exposed latency, not one per piece).  tid = threadIdx.x (a parameter so
// that the persistent backward can keep this addressing out of the registers that live across its tiles).
template <int ROWS, int KS, int NTHR>
__device__ __forceinline__ void stage_rows(unsigned char* dst, const bf16_t* src, long ld, long row0, long limit, int tid) {
    constexpr int CPR = KS * 4, NP = ROWS * CPR / NTHR;
    static_assert(ROWS * CPR % NTHR == 0, "tile must split evenly over the threads");
    u32x4_t v[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int idx = tid + NTHR * i;
        const int r = idx / CPR, c = idx - r * CPR;
        v[i] = u32x4_t{0, 0, 0, 0};
        if (row0 + r < limit) v[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(src + (row0 + r) * ld + c * 8));
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int idx = tid + NTHR * i;
        const int r = idx / CPR, c = idx - r * CPR;
        *reinterpret_cast<u32x4_t*>(dst + (c >> 2) * ROWS * 64 + slab_off(r, c & 3)) = v[i];
    }
}

// the residual pieces a thread adds in store_rows, requested ahead (during the last chunk) so that their HBM latency is not
// paid row by row in the store loop
template <int C, int NTHR> struct RowPre {
    static constexpr int P8 = C / 8, RG = NTHR / P8, NR = (64 + RG - 1) / RG;
};
template <int C, int NTHR> using PreArr = u32x4_t[BM / 64][RowPre<C, NTHR>::NR];
template <int C, int NTHR>
__device__ __forceinline__ void rows_prefetch(PreArr<C, NTHR>& v, const bf16_t* R, long ldr, long m0, long M) {
    using P = RowPre<C, NTHR>;
    const int c8 = threadIdx.x % P::P8, rg = threadIdx.x / P::P8;
#pragma unroll
    for (int piece = 0; piece < BM / 64; ++piece)
#pragma unroll
        for (int it = 0; it < P::NR; ++it) {
            const int row = rg + it * P::RG;
            const long m = m0 + piece * 64 + row;
            v[piece][it] = u32x4_t{0, 0, 0, 0};
            if (rg < P::RG && row < 64 && m < M) v[piece][it] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(R + m * ldr + c8 * 8));
        }
}

// fp32 accumulator tiles -> rows of Y through an LDS staging piece of 64 rows x (C + 4) floats, epilogue fused:
//   y = R + rowscale * (acc + bias)
// acc[tn][tm]: token row 16 tm + (lane & 15) of the wave's WROWS rows, columns wn * (C/2) + 16 tn + 4 (lane >> 4) .. +3
// KEEP: the accumulators stay in their registers until the barrier behind their ds_writes (for callers with LDS-DMA in flight)
template <int C, int NTHR, int NWM, int TM, bool KEEP = false>
__device__ __forceinline__ void store_rows(float* Cs, const f32x4_t (&acc)[C / 32][TM], int wm, int wn, int lane, long m0, long M,
                                           const float* bias, const float* rowscale, int rps, bool has_r,
                                           const PreArr<C, NTHR>& pre, bf16_t* Y, long ldy, int tid) {
    constexpr int LDC = C + 4, P8 = C / 8, RG = NTHR / P8, WROWS = 16 * TM, WPH = 64 / WROWS;   // waves (in m) per 64-row piece
    constexpr int NR = (64 + RG - 1) / RG;
    const int c8 = tid % P8, rg = tid / P8;
    float bv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = bias ? bias[c8 * 8 + j] : 0.f;
#pragma unroll
    for (int piece = 0; piece < NWM / WPH; ++piece) {
        if (piece) __syncthreads();
        if (wm / WPH == piece) {
#pragma unroll
            for (int tn = 0; tn < C / 32; ++tn)
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    const int row = (wm % WPH) * WROWS + 16 * tm + (lane & 15), col = wn * (C / 2) + 16 * tn + 4 * (lane >> 4);
                    *reinterpret_cast<f32x4_t*>(Cs + row * LDC + col) = acc[tn][tm];
                }
        }
        __syncthreads();
        if constexpr (KEEP) {
#pragma unroll
            for (int i = 0; i < (C / 32) * TM; ++i) asm volatile("" ::"v"(acc[i / TM][i % TM]));
        }
        if (rg < RG) {
#pragma unroll
            for (int it = 0; it < NR; ++it) {
                const int row = rg + it * RG;
                const long m = m0 + piece * 64 + row;
                if (row >= 64 || m >= M) break;
                const f32x4_t a = *reinterpret_cast<const f32x4_t*>(Cs + row * LDC + c8 * 8);
                const f32x4_t b = *reinterpret_cast<const f32x4_t*>(Cs + row * LDC + c8 * 8 + 4);
                float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] += bv[j];
                if (rowscale) {
                    const float s = rowscale[m / rps];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] *= s;
                }
                if (has_r) {
                    float r[8];
                    const u32x4_t q = pre[piece][it];
                    unpack8(make_uint4(q.x, q.y, q.z, q.w), r);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] += r[j];
                }
                store8_nt(Y + m * ldy + c8 * 8, v);
            }
        }
    }
}

// =================================================================================================================
// forward.  256 threads = 4 waves as 2 (tokens) x 2 (columns); chunk of HC hidden columns per round:
//   P1: h[128 x HC] = Xs . W1s^T (K = C)   -> + b1, GELU, bf16 -> As      (wave: 64 rows x HC/2)
//   P2: y[128 x C] += As . W2s^T (K = HC)                                   (wave: 64 rows x C/2)
// two barriers per round; the next chunk's weights travel global -> registers during P1 / P2
// =================================================================================================================
template <int C, int HC>
__global__ __launch_bounds__(256, 2) void mlp_fwd_kernel(const ga_mlp_desc d) {
    constexpr int KS1 = C / 32, KS2 = HC / 32, TN1 = HC / 32, TN2 = C / 32;
    constexpr int XS = KS1 * BM * 64, W1S = KS1 * HC * 64, AS = KS2 * BM * 64;
    constexpr int NI = HC * C / 8 / 256;                  // 16-byte weight pieces per thread and matrix
    static_assert(HC * C / 8 % 256 == 0, "weight chunk must split evenly");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* Xs = smem;
    unsigned char* W1s = Xs + XS;
    unsigned char* As = W1s + W1S;
    unsigned char* W2s = As + AS;
    float* B1s = reinterpret_cast<float*>(W2s + KS2 * C * 64);    // [4C]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, g = lane >> 4;
    const long m0 = (long)blockIdx.x * BM;
    const bf16_t* W1 = reinterpret_cast<const bf16_t*>(d.W1);
    const bf16_t* W2 = reinterpret_cast<const bf16_t*>(d.W2);

    u32x4_t w1r[NI], w2r[NI];
    auto w_load = [&](int j0) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int idx = tid + 256 * i;
            const int r1 = idx / (KS1 * 4), c1 = idx - r1 * (KS1 * 4);
            w1r[i] = *reinterpret_cast<const u32x4_t*>(W1 + (long)(j0 + r1) * d.ldw1 + c1 * 8);
            const int r2 = idx / (HC / 8), c2 = idx - r2 * (HC / 8);
            w2r[i] = *reinterpret_cast<const u32x4_t*>(W2 + (long)r2 * d.ldw2 + j0 + c2 * 8);
        }
    };
    auto w1_store = [&]() {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int idx = tid + 256 * i;
            const int r1 = idx / (KS1 * 4), c1 = idx - r1 * (KS1 * 4);
            *reinterpret_cast<u32x4_t*>(W1s + (c1 >> 2) * HC * 64 + slab_off(r1, c1 & 3)) = w1r[i];
        }
    };
    auto w2_store = [&]() {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int idx = tid + 256 * i;
            const int r2 = idx / (HC / 8), c2 = idx - r2 * (HC / 8);
            *reinterpret_cast<u32x4_t*>(W2s + (c2 >> 2) * C * 64 + slab_off(r2, c2 & 3)) = w2r[i];
        }
    };

    w_load(0);
    stage_rows<BM, KS1, 256>(Xs, reinterpret_cast<const bf16_t*>(d.X), d.ldx, m0, d.M, tid);
    for (int i = tid; i < 4 * C; i += 256) B1s[i] = d.b1[i];
    w1_store();
    w2_store();
    __syncthreads();

    f32x4_t y[TN2][4];
#pragma unroll
    for (int i = 0; i < TN2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) y[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // one round = one chunk of HC hidden columns; the last one (more = false) runs after the residual prefetch
    auto round = [&](const int j0, const bool more) __attribute__((always_inline)) {
        if (more) w_load(j0 + HC);
        // ---- P1
        f32x4_t h[TN1][4];
#pragma unroll
        for (int i = 0; i < TN1; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) h[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            bf16x8_t xf[4];
#pragma unroll
            for (int tm = 0; tm < 4; ++tm) xf[tm] = frag(Xs + ks * BM * 64, wm * 64 + 16 * tm, lane);
#pragma unroll
            for (int tn = 0; tn < TN1; ++tn) {
                const bf16x8_t wf = frag(W1s + ks * HC * 64, wn * (HC / 2) + 16 * tn, lane);
#pragma unroll
                for (int tm = 0; tm < 4; ++tm) h[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf[tm], h[tn][tm], 0, 0, 0);
            }
        }
#pragma unroll
        for (int tn = 0; tn < TN1; ++tn) {
            const int nl = wn * (HC / 2) + 16 * tn + 4 * g;              // first of this lane's 4 hidden columns in the chunk
            const float4 b = *reinterpret_cast<const float4*>(B1s + j0 + nl);
            const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int tm = 0; tm < 4; ++tm) {
                float a[4], unused;
#pragma unroll
                for (int r = 0; r < 4; ++r) gelu_both_fast(h[tn][tm][r] + bb[r], a[r], unused);
                const int row = wm * 64 + 16 * tm + (lane & 15);
                uint2 p;
                p.x = pack2bf(a[0], a[1]);
                p.y = pack2bf(a[2], a[3]);
                *reinterpret_cast<uint2*>(As + (nl >> 5) * BM * 64 + slab_off(row, (nl & 31) >> 3) + (nl & 7) * 2) = p;
            }
        }
        lds_barrier();                       // As complete; W1s is free
        // ---- P2
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) {
            bf16x8_t af[4];
#pragma unroll
            for (int tm = 0; tm < 4; ++tm) af[tm] = frag(As + ks * BM * 64, wm * 64 + 16 * tm, lane);
#pragma unroll
            for (int tn = 0; tn < TN2; ++tn) {
                const bf16x8_t wf = frag(W2s + ks * C * 64, wn * (C / 2) + 16 * tn, lane);
#pragma unroll
                for (int tm = 0; tm < 4; ++tm) y[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af[tm], y[tn][tm], 0, 0, 0);
            }
        }
        if (more) w1_store();                // its pieces had P1 + P2 to arrive from L2
        lds_barrier();                       // As / W2s are free, the new W1s is visible to everyone
        if (more) w2_store();                // read by P2 of the next round, after its first barrier
    };
    for (int j0 = 0; j0 + HC < d.H; j0 += HC) round(j0, true);
    u32x4_t rpre[BM / 64][RowPre<C, 256>::NR];
    if (d.R) rows_prefetch<C, 256>(rpre, reinterpret_cast<const bf16_t*>(d.R), d.ldr, m0, d.M);
    round(d.H - HC, false);
    // (the last barrier of the round has passed: every LDS operand is dead)
    store_rows<C, 256, 2, 4>(reinterpret_cast<float*>(smem), y, wm, wn, lane, m0, d.M, d.b2, d.rowscale, d.rows_per_scale,
                             d.R != nullptr, rpre, reinterpret_cast<bf16_t*>(d.Y), d.ldy, tid);
}

template <int C, int HC> constexpr int fwd_lds() {
    constexpr int ab = (C / 32) * BM * 64 + (C / 32) * HC * 64 + (HC / 32) * BM * 64 + (HC / 32) * C * 64 + 16 * C;
    constexpr int st = 64 * (C + 4) * 4;
    return ab > st ? ab : st;
}

// =================================================================================================================
// backward.  512 threads = 8 waves as 4 (tokens) x 2 (columns), one workgroup per CU (X and DY tiles both resident);
// per chunk of HC hidden columns:
//   P1: h = Xs . W1s^T,  t = Ds . W2Ts^T   (K = C; wave: 32 rows x HC/2 each)
//       a = gelu(h + b1) -> A2s,  dh = t * gelu'(h + b1) -> DHs
//   P2: dx[128 x C] += DHs . W1Ts^T (K = HC; wave: 32 rows x C/2);  A2s / DHs rows -> global with 16-byte stores
//       (a NULL A / DH: that tile is not stored)
// (measured at C = 96, M = 802816: 0.54 ms; a 4-wave / two-workgroup form writing a / dh as 8-byte pieces straight from the
//  accumulators: 1.06 ms -- the 32-byte runs cost more than the LDS staging)
//
// WG (desc.dW1 given, C = 96 only): the fc1 weight gradient dW1 += DH^T . X and db1 += colsum(DH) are accumulated here, from
// the DHs / Xs images that are in LDS anyway, so DH need not go to HBM and come back for a ga_wgrad launch.  The launch is then
// persistent: workgroup b walks the 128-row tiles b, b + grid, ... and keeps ONE accumulator set through all of them:
//   P2 also: dW1[j0 .. j0+HC)[0 .. C) += DHs^T . Xs (K = the tile's 128 token rows): 4 x 6 output tiles of 16 x 16 per chunk,
//       wave w owns hidden tile w >> 1 and channel tiles 3 (w & 1) .. +2, 4 k-steps of 32 rows.  Both operands are read
//       k-strided (rows = reduction index) out of the [row][64 B] slab images with ds_read_b64_tr_b16; db1 from the same DH
//       fragments (dot against ones, the TN GEMM's form), so it sums exactly the bf16 values the product multiplies.
//   Rows >= M of the last tile add nothing: stage_rows zero-fills Xs and Ds there, so t = 0 and dh = t * gelu' = 0.
//   The accumulators dw[chunk][3] (H / HC = 6 chunks, 72 VGPRs, + 6 for db1) are indexed statically: a scalar branch per chunk.
//   After its last tile the workgroup stores its fp32 partial [H*C + H] to part[b]; mlp_bwd_wg_reduce_kernel adds the
//   partials in workgroup order into dW1 / db1 (no float atomics: two runs give the same bits).
//   mlp_bwd_kernel<96, 64, true> (-Rpass-analysis=kernel-resource-usage): 241 VGPRs, 0 AGPRs, no VGPR / SGPR spill, no scratch,
//   2 waves per SIMD (the plain form: 158 VGPRs).  The rolled chunk loop and the laundered thread indices below are what keep it
//   there: unrolled six times the kernel spilled 239 registers, with running row pointers kept across the walk 45.
// =================================================================================================================
// byte offset, inside one [rows][64 B] slab, of this lane's piece of the transposed 4-row x 16-column block read
// (ds_read_b64_tr_b16: lane 4q + p of a 16-lane group supplies row q, columns 4p .. 4p+3 and receives column i of the 4 rows).
// Lane group g reads reduction rows 8g + 4hf .. +3 of a 32-row k-step: with hf = 0, 1 a lane ends up with rows 8g .. 8g+7 of
// column (lane & 15), the 16x16x32 operand.  u0 = first 16-byte unit of the 16 columns (0 or 2).  The swizzle term
// ((row >> 2) & 3) = (2g + hf) & 3 flips unit bits per lane group AND per half, so each (hf, u0) has an address of its own;
// k-steps (+ 32 rows) are a constant 2048 bytes apart.
__device__ __forceinline__ unsigned tr_off(int lane, int hf, int u0) {
    const int i = lane & 15, row = 8 * (lane >> 4) + 4 * hf + (i >> 2);
    return slab_off(row, u0 + ((i & 3) >> 1)) + 8 * (i & 1);
}
__device__ __forceinline__ bf16x8_t tr_frag(const unsigned char* lo, const unsigned char* hi) {
    s16x4_t v[2];
    v[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)lo);
    v[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)hi);
    return *reinterpret_cast<const bf16x8_t*>(&v[0]);
}

// PF (persistent form only, knob MLP_PREFETCH): the token rows of the NEXT tile of the walk travel while this one is computed.
//   A second X image (LDS 120,320 -> 144,896 B of 163,840): the two images swap roles per tile.  At the top of tile t the rows
//   of tile t + grid go into the spare image, and right behind the barrier that ends the last chunk's P1 -- the last reader of
//   Ds -- the DY rows of tile t + grid go into Ds.  Both by LDS-DMA (buffer_load_dwordx4 ... lds): wave w fills rows
//   16 w .. 16 w + 15 of each of the KS1 slabs, one 1 KiB wave-instruction per slab.  The DMA writes LDS lane-linearly, so the
//   slab_off XOR layout is made on the SOURCE side: lane l lands in unit slot l & 3 of row l >> 2 and therefore fetches unit
//   (l & 3) ^ ((l >> 4) & 3).  The buffer window is the tile's live rows exactly (base = row m0 of the operand, extent =
//   (rows - 1) ld + C elements), every offset is the lane's (the scalar offset takes no part in the range check): rows >= M
//   arrive as zeros, which is what stage_rows guarantees and the dW1 / dh = 0 reasoning above relies on.
//   Waits: the X rows are issued BEFORE chunk 0's w_load, so the wait the compiler places for those registers ahead of
//   w12_store retires them (vmcnt counts in order), and the barrier behind it shows them to every wave a whole tile before they
//   are read.  The DY rows are younger than the last chunk's w_load: the vmcnt(0) ahead of that chunk's w3_store retires them
//   (written out there as well), the barriers of the dx store and of the tile end follow.
//   The dx staging piece moves from smem + 0 (over Xs / Ds, both in use now) into DHs / A2s, dead after the last P2.
//   The first tile of a workgroup is staged by stage_rows as before.  No arithmetic changes: the same bits as PF = false.
//   No ds_write follows a DMA issue closely (global loads, fragment reads and MFMAs do), and the registers of the P1 / dx
//   staging ds_writes stay live up to the barrier behind them (the late ds_write data fetch recorded in DESIGN 5.3).
//   mlp_bwd_kernel<96, 64, true, true> (-Rpass-analysis=kernel-resource-usage): 245 VGPRs, 0 AGPRs, no VGPR spill, no scratch,
//   4 SGPRs spilled (to VGPR lanes: the two windows' scalars), 2 waves per SIMD; PF = false is instruction for instruction the
//   kernel it was before (241 VGPRs).  Measured (profiles/mlp_bwd_phases.txt, mlp_prefetch_ab.txt): the row staging was 17 % of a
//   stamped tile; 0.699 -> 0.633 ms per launch in the step.
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_s;
__device__ __forceinline__ u32x4_s rows_rsrc(const bf16_t* base, unsigned bytes) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(base);
    u32x4_s r;
    r[0] = __builtin_amdgcn_readfirstlane((unsigned)a);
    r[1] = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xffffu);
    r[2] = __builtin_amdgcn_readfirstlane(bytes);
    r[3] = 0x00020000u;
    return r;
}
// three LDS-DMA wave-instructions (64 lanes x 16 B each) to the wave-uniform LDS byte addresses dst, dst + 8 KiB, dst + 16 KiB
// (one per k slab) from the lane offsets v0 .. v2 of the window rs.  M0 carries the destination and is written in the statement
// that reads it; s_nop 4: the descriptor may come straight from v_readfirstlane.  Asm, so hipcc does not count the loads: see
// "Waits" above
__device__ __forceinline__ void dma_rows3(u32x4_s rs, unsigned v0, unsigned v1, unsigned v2, unsigned dst) {
    unsigned keep;
    asm volatile(
        "s_nop 4\n\ts_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %5\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %4, 0 offen lds\n\t"
        "s_mov_b32 m0, %6\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %4, 0 offen lds\n\t"
        "s_mov_b32 m0, %7\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %4, 0 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(v0), "v"(v1), "v"(v2), "s"(rs), "s"(dst), "s"(dst + 0x2000u), "s"(dst + 0x4000u)
        : "memory");
}

#ifdef GAEXT_MLP_STAMPS
constexpr int kMlpStamps = 5;     // stage, P1, P2 (+ dW1, a / dh rows, weight staging), dx store, tile-end barrier
// diagnostic build (make libgaext_stamps.so, tools/mlp_phases.py): clock stamps at the phase boundaries of the persistent walk, summed per
// workgroup and left behind the partials.  The fences forbid overlaps the real kernel has: read the shares, not the length
__device__ __forceinline__ unsigned long long mlp_stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define MLP_STAMP(k)                                  \
    do {                                              \
        const unsigned long long t_ = mlp_stamp();    \
        if constexpr (WG) st_sum[k] += t_ - st_prev;  \
        st_prev = t_;                                 \
    } while (0)
#else
#define MLP_STAMP(k) \
    do {             \
    } while (0)
#endif

template <int C, int HC, bool WG, bool PF = false>
__global__ __launch_bounds__(512, 1) void mlp_bwd_kernel(const ga_mlp_bwd_desc d) {
    constexpr int KS1 = C / 32, KS2 = HC / 32, TN1 = HC / 32, TN2 = C / 32;
    constexpr int XS = KS1 * BM * 64, WS = KS1 * HC * 64, TS = KS2 * BM * 64;
    constexpr int NPC = HC * C / 8, NI = (NPC + 511) / 512;     // 16-byte pieces per weight chunk / per thread
    constexpr int NCH = 4 * C / HC;                             // chunks of the hidden dimension (H = 4C)
    static_assert(!WG || (HC == 64 && C == 96), "the in-kernel weight gradient is laid out for 4 x 6 tiles over 8 waves");
    static_assert(!PF || (WG && KS1 == 3), "the prefetch belongs to the persistent walk; dma_rows3 fills three slabs");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // PF: X images at 0 and XS; xoff = the one this tile reads (every DMA destination stays below 72 KiB)
    unsigned xoff = 0;
    unsigned char* Ds = smem + (PF ? 2 : 1) * XS;
    unsigned char* W1s = Ds + XS;
    unsigned char* W2Ts = W1s + WS;
    unsigned char* W1Ts = W2Ts + WS;          // [C][HC]: KS2 slabs of C rows
    unsigned char* DHs = W1Ts + KS2 * C * 64;
    unsigned char* A2s = DHs + TS;
    float* B1s = reinterpret_cast<float*>(A2s + TS);               // [4C]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, g = lane >> 4;
    const bf16_t* W1 = reinterpret_cast<const bf16_t*>(d.W1);
    const bf16_t* W2T = reinterpret_cast<const bf16_t*>(d.W2T);
    const bf16_t* W1T = reinterpret_cast<const bf16_t*>(d.W1T);
    bf16_t* Aout = reinterpret_cast<bf16_t*>(d.A);
    bf16_t* DHout = reinterpret_cast<bf16_t*>(d.DH);

    u32x4_t w1r[NI], w2r[NI], w3r[NI];
    auto w_load = [&](int j0) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int idx = NPC % 512 == 0 ? tid + 512 * i : min(tid + 512 * i, NPC - 1);   // clamped: a few pieces twice
            const int r1 = idx / (KS1 * 4), c1 = idx - r1 * (KS1 * 4);
            w1r[i] = *reinterpret_cast<const u32x4_t*>(W1 + (long)(j0 + r1) * d.ldw1 + c1 * 8);
            w2r[i] = *reinterpret_cast<const u32x4_t*>(W2T + (long)(j0 + r1) * d.ldw2t + c1 * 8);
            const int r3 = idx / (HC / 8), c3 = idx - r3 * (HC / 8);
            w3r[i] = *reinterpret_cast<const u32x4_t*>(W1T + (long)r3 * d.ldw1t + j0 + c3 * 8);
        }
    };
    auto w12_store = [&]() {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int idx = NPC % 512 == 0 ? tid + 512 * i : min(tid + 512 * i, NPC - 1);
            const int r1 = idx / (KS1 * 4), c1 = idx - r1 * (KS1 * 4);
            const unsigned o = (c1 >> 2) * HC * 64 + slab_off(r1, c1 & 3);
            *reinterpret_cast<u32x4_t*>(W1s + o) = w1r[i];
            *reinterpret_cast<u32x4_t*>(W2Ts + o) = w2r[i];
        }
    };
    auto w3_store = [&]() {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int idx = NPC % 512 == 0 ? tid + 512 * i : min(tid + 512 * i, NPC - 1);
            const int r3 = idx / (HC / 8), c3 = idx - r3 * (HC / 8);
            *reinterpret_cast<u32x4_t*>(W1Ts + (c3 >> 2) * C * 64 + slab_off(r3, c3 & 3)) = w3r[i];
        }
    };

    // WG: this wave's share of the weight gradient, kept through every tile the workgroup walks
    constexpr int NDW = WG ? NCH : 1;
    f32x4_t dw[NDW][3];
    float bsum[NDW];
    unsigned tra[2];                           // lane part of the transposed fragment read addresses, per 4-row half
    if constexpr (WG) {
#pragma unroll
        for (int i = 0; i < NDW; ++i) {
            bsum[i] = 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) dw[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        tra[0] = tr_off(lane, 0, 0);
        tra[1] = tr_off(lane, 1, 0);
    }
    // wave-uniform part: slab and first unit of a 16-column block; units 2, 3 are units 0, 1 with address bit 5 flipped
    const int wu = __builtin_amdgcn_readfirstlane(wave);
    auto tr_blk = [&](const unsigned char* img, int blk, int ks) __attribute__((always_inline)) {
        const unsigned o = (unsigned)(img - smem) + (blk >> 1) * BM * 64 + ks * 2048, x = (blk & 1) << 5;
        return tr_frag(smem + ((tra[0] ^ x) + o), smem + ((tra[1] ^ x) + o));
    };

    for (int i = tid; i < 4 * C; i += 512) B1s[i] = d.b1[i];
    const long ntiles = (d.M + BM - 1) / BM;
    long tile = blockIdx.x;
#ifdef GAEXT_MLP_STAMPS
    unsigned long long st_sum[kMlpStamps] = {0, 0, 0, 0, 0}, st_prev = mlp_stamp();
#endif
    // PF: the 128 rows of tile t + grid of `src` -> the slab images at `dst`; rows >= M read as zeros (window = the live rows)
    auto dma_next = [&](const void* src, long ld, unsigned char* dst) __attribute__((always_inline)) {
        const long mn = (tile + (long)gridDim.x) * BM;
        const long live = d.M - mn < BM ? d.M - mn : BM;
        const u32x4_s rs = rows_rsrc(reinterpret_cast<const bf16_t*>(src) + mn * ld, (unsigned)(((live - 1) * ld + C) * 2));
        int dtid = tid;
        asm volatile("" : "+v"(dtid));
        const int l = dtid & 63;
        const unsigned v = (unsigned)((16 * wu + (l >> 2)) * (int)ld * 2 + (((l & 3) ^ ((l >> 4) & 3)) << 4));
        const unsigned lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)dst;
        dma_rows3(rs, v, v + 64, v + 128, __builtin_amdgcn_readfirstlane(lds + wu * 1024));
    };
    // the rows of tile m0 through registers, with the workgroup's first tile the weights of chunk 0 (later tiles: staged by the
    // previous tile's last chunk).  WG: the per-tile addressing (row staging, DX rows) is derived from a copy of the thread index
    // that the compiler cannot see through, so it is re-computed per tile and not kept -- spilled -- across the whole tile walk
    auto stage_tile = [&](unsigned char* Xs, const long m0, const bool first) __attribute__((always_inline)) {
        int ttid = tid;
        if constexpr (WG) asm volatile("" : "+v"(ttid));
        stage_rows<BM, KS1, 512>(Xs, reinterpret_cast<const bf16_t*>(d.X), d.ldx, m0, d.M, ttid);
        stage_rows<BM, KS1, 512>(Ds, reinterpret_cast<const bf16_t*>(d.DY), d.lddy, m0, d.M, ttid);
        if (first) {
            w12_store();
            w3_store();
        }
        __syncthreads();
    };
    w_load(0);
    if constexpr (PF) stage_tile(smem, tile * BM, true);      // every later tile arrives by DMA
    while (true) {
        const long m0 = tile * BM;
        const bool next_tile = WG && tile + (long)gridDim.x < ntiles;
        unsigned char* const Xs = smem + xoff;
        if constexpr (!PF) stage_tile(Xs, m0, !WG || tile == (long)blockIdx.x);
        MLP_STAMP(0);
        // (PF, later tiles: the rows came by DMA and the tile-end barrier below has shown them to every wave)
        if constexpr (PF) {
            if (next_tile) dma_next(d.X, d.ldx, smem + (xoff ^ XS));
        }

        f32x4_t dx[TN2][2];
#pragma unroll
        for (int i = 0; i < TN2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) dx[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

        // one chunk of HC hidden columns; `more`: stage the weights of chunk jn behind it
        // this wave's 3 tiles of dW1 rows [j0 + 16 jt, + 16) from the chunk's DHs and the tile's Xs.  Rows = hidden (first
        // operand), columns = channels; every lane takes part in every read (the transposing read needs EXEC all ones), only
        // the bias dot is wave-conditional
        auto wg_chunk = [&](f32x4_t (&dwc)[3], float& bs) __attribute__((always_inline)) {
            typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
            const bf16x2_t ones2 = {(__bf16)1.0f, (__bf16)1.0f};
#pragma unroll
            for (int ks = 0; ks < BM / 32; ++ks) {
                const bf16x8_t hf8 = tr_blk(DHs, wu >> 1, ks);
#pragma unroll
                for (int tc = 0; tc < 3; ++tc) {
                    const bf16x8_t xf8 = tr_blk(Xs, 3 * (wu & 1) + tc, ks);
                    dwc[tc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hf8, xf8, dwc[tc], 0, 0, 0);
                }
                if ((wu & 1) == 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        bs = __builtin_amdgcn_fdot2_f32_bf16(bf16x2_t{hf8[2 * j], hf8[2 * j + 1]}, ones2, bs, false);
                }
            }
        };
        // dy_next (PF): this is the tile's last chunk and the walk goes on -- Ds is refilled behind the P1 barrier
        auto chunk = [&](const int j0, const bool more, const int jn, const bool dy_next) __attribute__((always_inline)) {
            if (more) w_load(jn);
            // ---- P1
            f32x4_t h[TN1][2], t[TN1][2];
            [[maybe_unused]] uint2 pkeep[TN1][2][2];
#pragma unroll
            for (int i = 0; i < TN1; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) h[i][j] = t[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) {
                bf16x8_t xf[2], df[2];
#pragma unroll
                for (int tm = 0; tm < 2; ++tm) {
                    xf[tm] = frag(Xs + ks * BM * 64, wm * 32 + 16 * tm, lane);
                    df[tm] = frag(Ds + ks * BM * 64, wm * 32 + 16 * tm, lane);
                }
#pragma unroll
                for (int tn = 0; tn < TN1; ++tn) {
                    const bf16x8_t w1f = frag(W1s + ks * HC * 64, wn * (HC / 2) + 16 * tn, lane);
                    const bf16x8_t w2f = frag(W2Ts + ks * HC * 64, wn * (HC / 2) + 16 * tn, lane);
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm) {
                        h[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1f, xf[tm], h[tn][tm], 0, 0, 0);
                        t[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2f, df[tm], t[tn][tm], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int tn = 0; tn < TN1; ++tn) {
                const int nl = wn * (HC / 2) + 16 * tn + 4 * g;
                const float4 b = *reinterpret_cast<const float4*>(B1s + j0 + nl);
                const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int tm = 0; tm < 2; ++tm) {
                    float a[4], dh[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float gr;
                        gelu_both_fast(h[tn][tm][r] + bb[r], a[r], gr);
                        dh[r] = t[tn][tm][r] * gr;
                    }
                    const int row = wm * 32 + 16 * tm + (lane & 15);
                    const unsigned o = (nl >> 5) * BM * 64 + slab_off(row, (nl & 31) >> 3) + (nl & 7) * 2;
                    uint2 p;
                    p.x = pack2bf(a[0], a[1]);
                    p.y = pack2bf(a[2], a[3]);
                    *reinterpret_cast<uint2*>(A2s + o) = p;
                    if constexpr (PF) pkeep[tn][tm][0] = p;
                    p.x = pack2bf(dh[0], dh[1]);
                    p.y = pack2bf(dh[2], dh[3]);
                    *reinterpret_cast<uint2*>(DHs + o) = p;
                    if constexpr (PF) pkeep[tn][tm][1] = p;
                }
            }
            lds_barrier();                       // A2s / DHs complete; W1s / W2Ts are free
            if constexpr (PF) {
                // the written pieces stay in their registers until the writes are done (X rows may still be arriving by DMA)
#pragma unroll
                for (int i = 0; i < TN1 * 4; ++i) asm volatile("" ::"v"(pkeep[i >> 2][(i >> 1) & 1][i & 1].x), "v"(pkeep[i >> 2][(i >> 1) & 1][i & 1].y));
                // Ds had its last reader in the P1 above
                if (dy_next) dma_next(d.DY, d.lddy, Ds);
            }
            MLP_STAMP(1);
            // ---- P2
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) {
                bf16x8_t af[2];
#pragma unroll
                for (int tm = 0; tm < 2; ++tm) af[tm] = frag(DHs + ks * BM * 64, wm * 32 + 16 * tm, lane);
#pragma unroll
                for (int tn = 0; tn < TN2; ++tn) {
                    const bf16x8_t wf = frag(W1Ts + ks * C * 64, wn * (C / 2) + 16 * tn, lane);
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm) dx[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af[tm], dx[tn][tm], 0, 0, 0);
                }
            }
            if constexpr (WG) {
                // the chunk loop stays rolled (unrolled, its six copies of the weight addressing spill); the accumulator set of
                // the chunk is chosen by a scalar branch so that every register index is static
                static_assert(NDW == 1 || NDW == 6, "one case per chunk");
                switch (j0 / HC) {
                    case 0: wg_chunk(dw[0], bsum[0]); break;
                    case 1: wg_chunk(dw[1 % NDW], bsum[1 % NDW]); break;
                    case 2: wg_chunk(dw[2 % NDW], bsum[2 % NDW]); break;
                    case 3: wg_chunk(dw[3 % NDW], bsum[3 % NDW]); break;
                    case 4: wg_chunk(dw[4 % NDW], bsum[4 % NDW]); break;
                    default: wg_chunk(dw[5 % NDW], bsum[5 % NDW]); break;
                }
            }
            // rows of a / dh of this chunk -> global (HC bf16 = HC/8 16-byte pieces per row)
            if (Aout || DHout) {
                constexpr int PPR = HC / 8, NP = BM * PPR / 512;
                static_assert(BM * PPR % 512 == 0, "chunk rows must split evenly");
                int ctid = tid;                  // WG: as ttid above -- no running row pointers across chunks and tiles
                if constexpr (WG) asm volatile("" : "+v"(ctid));
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const int idx = ctid + 512 * i;
                    const int r = idx / PPR, c = idx - r * PPR;
                    const long m = m0 + r;
                    if (m < d.M) {
                        const unsigned o = (c >> 2) * BM * 64 + slab_off(r, c & 3);
                        if (Aout) store16_nt(Aout + m * d.lda + j0 + c * 8, *reinterpret_cast<const uint4*>(A2s + o));
                        if (DHout) store16_nt(DHout + m * d.lddh + j0 + c * 8, *reinterpret_cast<const uint4*>(DHs + o));
                    }
                }
            }
            if (more) w12_store();
            lds_barrier();                       // A2s / DHs / W1Ts are free, the new W1s / W2Ts visible
            if (more) w3_store();
            if constexpr (PF) {
                // counts every vector memory operation of the wave, and adds no wait: w3_store has just waited for the youngest
                // weight register with vmcnt(0) (the a / dh stores behind it are conditional, so the compiler counts none).
                // Written out because the DY rows, issued BEHIND this chunk's w_load, are retired by that wait alone; the
                // store_rows barriers and the tile-end barrier then show them to every wave
                if (dy_next) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            MLP_STAMP(2);
        };
        for (int j0 = 0; j0 < d.H; j0 += HC) {
            const bool last = j0 + HC >= d.H;
            // PF: chunk 0's weights are staged behind the workgroup's last chunk as well (unused).  With `more` a constant the
            // compiler follows the weight registers from load to store on one path; as a condition it sees loads pending at
            // the head of the next chunk and drains vmcnt there -- the rows in flight with it
            chunk(j0, PF || !last || next_tile, last ? 0 : j0 + HC, last && next_tile);
        }
        u32x4_t nopre[BM / 64][RowPre<C, 512>::NR];
#pragma unroll
        for (int i = 0; i < BM / 64; ++i)
#pragma unroll
            for (int j = 0; j < RowPre<C, 512>::NR; ++j) nopre[i][j] = u32x4_t{0, 0, 0, 0};
        // (the staging piece covers Xs and the head of Ds only: the weights staged for the next tile are beyond it.
        //  PF: it lies in DHs / A2s, 25,600 of their 32,768 bytes -- Xs, the spare image and Ds all hold or receive rows)
        static_assert(!PF || 64 * (C + 4) * 4 <= 2 * TS, "the dx staging piece must fit into DHs + A2s");
        int stid = tid;
        if constexpr (WG) asm volatile("" : "+v"(stid));
        store_rows<C, 512, 4, 2, PF>(reinterpret_cast<float*>(PF ? DHs : smem), dx, stid >> 7, (stid >> 6) & 1, stid & 63, m0, d.M, nullptr,
                                     nullptr, 1, false, nopre, reinterpret_cast<bf16_t*>(d.DX), d.lddx, stid);
        MLP_STAMP(3);
        if (!next_tile) break;
        if constexpr (PF) xoff ^= XS;
        tile += gridDim.x;
        __syncthreads();                         // the staging piece has been read: Xs / Ds may be staged again (PF: hold the rows)
        MLP_STAMP(4);
    }
#ifdef GAEXT_MLP_STAMPS
    if constexpr (WG) {
        // behind the partials of all workgroups, where the caller left the room (tools/mlp_phases.py does)
        unsigned long long* sp = reinterpret_cast<unsigned long long*>(d.partials + (long)gridDim.x * (4 * C * C + 4 * C)) +
                                 (long)blockIdx.x * kMlpStamps;
        if (tid == 0 && d.partials_bytes >= (size_t)gridDim.x * ((4 * C * C + 4 * C) * sizeof(float) + kMlpStamps * 8))
            for (int i = 0; i < kMlpStamps; ++i) sp[i] = st_sum[i];
    }
#endif
    if constexpr (WG) {
        // lane: channel = column (lane & 15) of the tile, hidden rows 4 g + r
        float* P = d.partials + (long)blockIdx.x * (4 * C * C + 4 * C);
        int etid = tid;
        asm volatile("" : "+v"(etid));
        const int lane = etid & 63, g = lane >> 4, jt = wu >> 1;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int tc = 0; tc < 3; ++tc)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    P[(ch * HC + 16 * jt + 4 * g + r) * C + 16 * (3 * (wu & 1) + tc) + (lane & 15)] = dw[ch][tc][r];
            float v = bsum[ch];                  // hidden column (lane & 15); the 4 lane groups hold row subsets
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if ((wu & 1) == 0 && lane < 16) P[4 * C * C + ch * HC + 16 * jt + lane] = v;
        }
    }
}

// dW1[j][c] += sum_b part[b][j * C + c],  db1[j] += sum_b part[b][H * C + j], b in workgroup order whatever the grid: thread
// group q of 4 sums the partials q, q + 4, ..., then the four sums are added in order.  n = H*C + H, a multiple of 4, as is C.
__global__ __launch_bounds__(256) void mlp_bwd_wg_reduce_kernel(const float* __restrict__ part, int nparts, int n, int nw, int C,
                                                                float* __restrict__ dW1, long ldw, float* __restrict__ db1) {
    __shared__ float4 sh[3][64];
    const int q = threadIdx.x >> 6;
    const long i = ((long)blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) {
#pragma unroll 4
        for (int s = q; s < nparts; s += 4) {
            const float4 b = *reinterpret_cast<const float4*>(part + (long)s * n + i);
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
    }
    if (q) sh[q - 1][threadIdx.x & 63] = a;
    __syncthreads();
    if (q || i >= n) return;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const float4 b = sh[s][threadIdx.x];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    float* dst = i < nw ? dW1 + (i / C) * ldw + (i % C) : db1 + (i - nw);
    dst[0] += a.x; dst[1] += a.y; dst[2] += a.z; dst[3] += a.w;
}

template <int C, int HC> constexpr int bwd_lds() {
    return 2 * (C / 32) * BM * 64 + 2 * (C / 32) * HC * 64 + (HC / 32) * C * 64 + 2 * (HC / 32) * BM * 64 + 16 * C;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename K> bool set_lds(K kern, size_t bytes) {
    return bytes <= 65536 ||
           hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

}  // namespace

extern "C" int ga_mlp_supported(int C, int H, int dtype) { return dtype == GA_BF16 && H == 4 * C && (C == 96 || C == 192); }

extern "C" int ga_mlp_fwd(const ga_mlp_desc* d, ga_stream_t stream) {
    GA_REQUIRE(d && d->X && d->W1 && d->b1 && d->W2 && d->Y && d->M > 0, "ga_mlp_fwd: null / empty descriptor");
    GA_REQUIRE(ga_mlp_supported(d->C, d->H, d->dtype), "ga_mlp_fwd: C=%d H=%d dtype=%d has no fused form (ga_mlp_supported)", d->C,
               d->H, d->dtype);
    GA_REQUIRE(aligned16(d->X) && aligned16(d->W1) && aligned16(d->W2) && aligned16(d->Y) && aligned16(d->b1) &&
                   (!d->R || aligned16(d->R)) && d->ldx % 8 == 0 && d->ldw1 % 8 == 0 && d->ldw2 % 8 == 0 && d->ldy % 8 == 0 &&
                   (!d->R || d->ldr % 8 == 0) && d->ldx >= d->C && d->ldw1 >= d->C && d->ldw2 >= d->H && d->ldy >= d->C,
               "ga_mlp_fwd: operands must be 16-byte aligned with leading dimensions in multiples of 8");
    GA_REQUIRE(!d->rowscale || d->rows_per_scale > 0, "ga_mlp_fwd: rows_per_scale");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)((d->M + BM - 1) / BM);
    if (d->C == 96) {
        constexpr int lds = fwd_lds<96, 64>();
        GA_REQUIRE(set_lds(mlp_fwd_kernel<96, 64>, lds), "ga_mlp_fwd: LDS");
        hipLaunchKernelGGL((mlp_fwd_kernel<96, 64>), dim3(grid), dim3(256), lds, s, *d);
    } else {
        constexpr int lds = fwd_lds<192, 32>();
        GA_REQUIRE(set_lds(mlp_fwd_kernel<192, 32>, lds), "ga_mlp_fwd: LDS");
        hipLaunchKernelGGL((mlp_fwd_kernel<192, 32>), dim3(grid), dim3(256), lds, s, *d);
    }
    return ga_check_launch("ga_mlp_fwd");
}

extern "C" int ga_mlp_bwd_wgrad_supported(int C, int H, int dtype) { return dtype == GA_BF16 && C == 96 && H == 4 * C; }

namespace {

// persistent grid of the weight-gradient form: the workgroups that are resident at once (occupancy query, as the ring GEMM
// does it), at most max_blocks when that is given, and never more than there are tiles -- so no workgroup is without a tile
// and every partial is written.  0: the LDS cannot be reserved.
int wg_grid(const ga_mlp_bwd_desc* d) {
    constexpr int lds = bwd_lds<96, 64>();
    static const int resident = [] {
        auto kern = mlp_bwd_kernel<96, 64, true>;
        if (!set_lds(kern, lds)) return 0;
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, 512, lds) != hipSuccess || n < 1) n = 1;
        return n * ga_num_cus();
    }();
    long grid = resident;
    if (d->max_blocks > 0) grid = std::min<long>(grid, d->max_blocks);
    return (int)std::min<long>(grid, (d->M + BM - 1) / BM);
}

}  // namespace

extern "C" size_t ga_mlp_bwd_partials(const ga_mlp_bwd_desc* d) {
    if (!d || d->M <= 0 || !ga_mlp_bwd_wgrad_supported(d->C, d->H, d->dtype)) return 0;
    return (size_t)wg_grid(d) * ((size_t)d->H * d->C + d->H) * sizeof(float);
}

extern "C" int ga_mlp_bwd(const ga_mlp_bwd_desc* d, ga_stream_t stream) {
    GA_REQUIRE(d && d->X && d->DY && d->W1 && d->b1 && d->W2T && d->W1T && d->DX && d->M > 0, "ga_mlp_bwd: null / empty descriptor");
    GA_REQUIRE(ga_mlp_supported(d->C, d->H, d->dtype), "ga_mlp_bwd: C=%d H=%d dtype=%d has no fused form (ga_mlp_supported)", d->C,
               d->H, d->dtype);
    GA_REQUIRE(aligned16(d->X) && aligned16(d->DY) && aligned16(d->W1) && aligned16(d->W2T) && aligned16(d->W1T) &&
                   aligned16(d->A) && aligned16(d->DH) && aligned16(d->DX) && aligned16(d->b1) && d->ldx % 8 == 0 &&
                   d->lddy % 8 == 0 && d->ldw1 % 8 == 0 && d->ldw2t % 8 == 0 && d->ldw1t % 8 == 0 && (!d->A || d->lda % 8 == 0) &&
                   (!d->DH || d->lddh % 8 == 0) && d->lddx % 8 == 0 && d->ldx >= d->C && d->lddy >= d->C && d->ldw1 >= d->C &&
                   d->ldw2t >= d->C && d->ldw1t >= d->H && (!d->A || d->lda >= d->H) && (!d->DH || d->lddh >= d->H) &&
                   d->lddx >= d->C,
               "ga_mlp_bwd: operands must be 16-byte aligned with leading dimensions in multiples of 8");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (d->dW1) {
        // fc1 weight gradient accumulated in the kernel (persistent launch) + the fixed-order sum of the workgroups' partials
        GA_REQUIRE(ga_mlp_bwd_wgrad_supported(d->C, d->H, d->dtype),
                   "ga_mlp_bwd: dW1 is accumulated in the kernel at C=96 only, not C=%d H=%d dtype=%d (ga_mlp_bwd_wgrad_supported)",
                   d->C, d->H, d->dtype);
        GA_REQUIRE(d->db1 && d->partials && aligned16(d->partials) && d->ldw >= d->C && d->max_blocks >= 0,
                   "ga_mlp_bwd: dW1 needs db1, 16-byte aligned partials and ldw >= C");
        constexpr int lds = bwd_lds<96, 64>();
        const int grid = wg_grid(d);
        GA_REQUIRE(grid > 0, "ga_mlp_bwd: LDS");
        const int n = d->H * d->C + d->H;
        GA_REQUIRE(d->partials_bytes >= (size_t)grid * n * sizeof(float), "ga_mlp_bwd: partials holds %zu bytes, %zu needed (ga_mlp_bwd_partials)",
                   (size_t)d->partials_bytes, (size_t)grid * n * sizeof(float));
        // MLP_PREFETCH (default 1): the next tile's rows travel by LDS-DMA during this one (PF above); 0: every tile through
        // stage_rows.  Same grid, same tile walk, same bits
        if (GA_KNOB("MLP_PREFETCH", 1)) {
            constexpr int lds_pf = lds + (96 / 32) * BM * 64;          // the second X image
            static const bool pf_ok = set_lds(mlp_bwd_kernel<96, 64, true, true>, lds_pf);
            GA_REQUIRE(pf_ok, "ga_mlp_bwd: LDS (MLP_PREFETCH)");
            hipLaunchKernelGGL((mlp_bwd_kernel<96, 64, true, true>), dim3(grid), dim3(512), lds_pf, s, *d);
        } else {
            hipLaunchKernelGGL((mlp_bwd_kernel<96, 64, true>), dim3(grid), dim3(512), lds, s, *d);
        }
        hipLaunchKernelGGL(mlp_bwd_wg_reduce_kernel, dim3((n / 4 + 63) / 64), dim3(256), 0, s, d->partials, grid, n, d->H * d->C, d->C,
                           d->dW1, (long)d->ldw, d->db1);
        return ga_check_launch("ga_mlp_bwd");
    }
    const unsigned grid = (unsigned)((d->M + BM - 1) / BM);
    if (d->C == 96) {
        constexpr int lds = bwd_lds<96, 64>();
        GA_REQUIRE(set_lds(mlp_bwd_kernel<96, 64, false>, lds), "ga_mlp_bwd: LDS");
        hipLaunchKernelGGL((mlp_bwd_kernel<96, 64, false>), dim3(grid), dim3(512), lds, s, *d);
    } else {
        constexpr int lds = bwd_lds<192, 32>();
        GA_REQUIRE(set_lds(mlp_bwd_kernel<192, 32, false>, lds), "ga_mlp_bwd: LDS");
        hipLaunchKernelGGL((mlp_bwd_kernel<192, 32, false>), dim3(grid), dim3(512), lds, s, *d);
    }
    return ga_check_launch("ga_mlp_bwd");
}
