// Few-row forms of ga_gemm (NT) and ga_wgrad (TN): the products of the model heads that have one row per image (M = batch = 256).
//
// The tall forms of gemm.hip give such a launch 128-row tiles: a 256 x 192 x 768 product becomes 4 workgroups on a 256-CU chip,
// each walking its K stages one global-load latency at a time.  Nothing here is near a memory or MFMA limit -- a launch moves a
// few MB and at most 1 GFLOP -- so the tile comes from the latency argument instead: many small workgroups, every load of a
// wave's share issued before its first wait.  Plain C++ (no inline assembly, nothing for the load audit), bf16 only; what the
// kernels do not take is forwarded to ga_gemm / ga_wgrad unchanged (gemm_select.h: nt_fewrows_wanted / tn_fewrows_wanted).
//
//  * NT (C = A B^T): one 256-thread workgroup per 32 x 32 output tile and batch element.  Both operands are K-contiguous, so a
//    lane's MFMA fragment (8 consecutive k of one row) is ONE 16-byte global load and nothing is staged through LDS.  The four
//    waves split K; each wave walks its share in chunks of 4 k-steps (128 elements of K), the next chunk's 16 loads in flight
//    while this one is multiplied.  The four partial tiles meet in 16 KiB of LDS and the epilogue runs once, 4 columns per thread.
//    The weight fragment is the MFMA "A" operand, as in gemm.hip, so a lane holds 4 consecutive output columns of one row.
//  * TN (dW = Y^T X): one workgroup per 64 x 64 output tile and batch element, the whole reduction over M inside it, so no atomics
//    between workgroups and no split_m: the result is the same bits from run to run.  128 reduction rows at a time go through one
//    [128][256 B] LDS image (Y columns in the first 128 bytes of a row, X columns in the second) in gemm_tn_kernel's XOR layout,
//    read back with the transposing ds_read_b64_tr_b16; the next 128 rows are in registers meanwhile.
#include <algorithm>
#include "common.h"
#include "gemm_select.h"

namespace {

using namespace gasel;

constexpr int kFrThreads = 256;
constexpr int kFrChunk = 4;        // k-steps of 32 per chunk of the NT wave loop

__device__ __forceinline__ uint4 fr_zero4() { return make_uint4(0u, 0u, 0u, 0u); }

// ================================================================================================
// NT, 32 x 32 tile
// ================================================================================================
struct FrFrag {
    uint4 a[2][kFrChunk], b[2][kFrChunk];      // [16-row block][k-step]: rows of A (output rows) / of B (output columns)
};

__global__ __launch_bounds__(kFrThreads) void gemm_nt_fewrows_kernel(const ga_gemm_desc d) {
    __shared__ __attribute__((aligned(16))) float part[4][32 * 32];      // per wave: [row][4-column group ^ (row & 7)]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_n = (d.N + 31) >> 5;
    const int tile_m = blockIdx.x / tiles_n, tile_n = blockIdx.x - tile_m * tiles_n;
    const int m0 = tile_m * 32, n0 = tile_n * 32;
    const long z = blockIdx.z;
    const long za = d.a_batch_mod > 0 ? z % d.a_batch_mod : z;
    const bf16_t* Ab = reinterpret_cast<const bf16_t*>(d.A) + za * d.strideA;
    const bf16_t* Bb = reinterpret_cast<const bf16_t*>(d.B) + z * d.strideB;

    // fragment rows: rows past the edge read the last row (their results are never stored), k past the edge reads zeros
    const int fr = lane & 15, kq = (lane >> 4) * 8;
    const bf16_t* Ap[2];
    const bf16_t* Bp[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        Ap[i] = Ab + (long)min(m0 + 16 * i + fr, d.M - 1) * d.lda;
        Bp[i] = Bb + (long)min(n0 + 16 * i + fr, d.N - 1) * d.ldb;
    }
    const int nsteps = (d.K + 31) >> 5, per = (nsteps + 3) >> 2;
    const int s0 = wave * per, s1 = min(s0 + per, nsteps);
    const int nchunks = s1 > s0 ? (s1 - s0 + kFrChunk - 1) / kFrChunk : 0;

    auto load = [&](int c, FrFrag& f) {
#pragma unroll
        for (int i = 0; i < kFrChunk; ++i) {
            const int s = s0 + c * kFrChunk + i, k = s * 32 + kq;
            const bool ok = s < s1 && k < d.K;       // K % 8 == 0: a lane's 8 elements are all inside or all outside
            const int kk = ok ? k : 0;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint4 va = *reinterpret_cast<const uint4*>(Ap[j] + kk);
                const uint4 vb = *reinterpret_cast<const uint4*>(Bp[j] + kk);
                f.a[j][i] = ok ? va : fr_zero4();
                f.b[j][i] = ok ? vb : fr_zero4();
            }
        }
    };
    f32x4_t acc[2][2];      // [column block][row block]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    auto mma = [&](const FrFrag& f) {
#pragma unroll
        for (int i = 0; i < kFrChunk; ++i)
#pragma unroll
            for (int bn = 0; bn < 2; ++bn)
#pragma unroll
                for (int bm = 0; bm < 2; ++bm)
                    acc[bn][bm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(&f.b[bn][i]),
                                                                          *reinterpret_cast<const bf16x8_t*>(&f.a[bm][i]),
                                                                          acc[bn][bm], 0, 0, 0);
    };
    FrFrag f0, f1;
    if (nchunks > 0) load(0, f0);
    for (int c = 0; c < nchunks; c += 2) {
        if (c + 1 < nchunks) load(c + 1, f1);
        mma(f0);
        if (c + 1 < nchunks) {
            if (c + 2 < nchunks) load(c + 2, f0);
            mma(f1);
        }
    }

    // D[row = column index (lane >> 4) * 4 + r][col = row index lane & 15]: 4 consecutive output columns of one output row
#pragma unroll
    for (int bn = 0; bn < 2; ++bn)
#pragma unroll
        for (int bm = 0; bm < 2; ++bm) {
            const int row = bm * 16 + (lane & 15), c4 = bn * 4 + (lane >> 4);
            *reinterpret_cast<f32x4_t*>(&part[wave][row * 32 + ((c4 ^ (row & 7)) << 2)]) = acc[bn][bm];
        }
    __syncthreads();

    // ---- epilogue, once: thread = one row x 4 columns; the order is ga_gemm's (include/gaext.h)
    const int row = tid >> 3, c4 = tid & 7;
    const long m = m0 + row;
    const int n = n0 + c4 * 4;
    float v[4];
    {
        const int o = row * 32 + ((c4 ^ (row & 7)) << 2);
        const f32x4_t p0 = *reinterpret_cast<const f32x4_t*>(&part[0][o]), p1 = *reinterpret_cast<const f32x4_t*>(&part[1][o]);
        const f32x4_t p2 = *reinterpret_cast<const f32x4_t*>(&part[2][o]), p3 = *reinterpret_cast<const f32x4_t*>(&part[3][o]);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (p0[j] + p1[j]) + (p2[j] + p3[j]);
    }
    const bool live = m < d.M && n < d.N;
    const bool full = n + 3 < d.N;
    float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const float* bias = d.bias ? d.bias + z * d.strideBias : nullptr;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] * d.alpha + ((bias && n + j < d.N) ? bias[n + j] : 0.f);
        const long coff = z * d.strideC + m * d.ldc + n;
        if (d.act == GA_ACT_GELU) {      // fc1: gelu (and gelu' into C2), the logistic form of the bf16 fc1 epilogue
            float w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) gelu_both_fast(v[j], v[j], w[j]);
            if (d.C2) {
                bf16_t* C2p = reinterpret_cast<bf16_t*>(d.C2) + coff;
                if (full) {
                    store4(C2p, w);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (n + j < d.N) C2p[j] = f2bf(w[j]);
                }
            }
        }
        if (d.H) {                       // dgrad2: times the stored GELU'
            const bf16_t* Hp = reinterpret_cast<const bf16_t*>(d.H) + z * d.strideH + m * d.ldh + n;
            float h[4] = {0.f, 0.f, 0.f, 0.f};
            if (full) {
                load4(Hp, h);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n + j < d.N) h[j] = bf2f(Hp[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= h[j];
        }
        if (d.rowscale) {
            const float s = d.rowscale[(unsigned)m / (unsigned)d.rows_per_scale];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= s;
        }
        if (d.R) {
            const bf16_t* Rp = reinterpret_cast<const bf16_t*>(d.R) + z * d.strideR + m * d.ldr + n;
            float r[4] = {0.f, 0.f, 0.f, 0.f};
            if (full) {
                load4(Rp, r);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n + j < d.N) r[j] = bf2f(Rp[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += r[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n + j < d.N) {
                cs[j] = v[j];
                cq[j] = v[j] * v[j];
            }
        if (d.c_f32) {
            float* Cp = reinterpret_cast<float*>(d.C) + coff;
            if (full) {
                store4(Cp, v);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n + j < d.N) Cp[j] = v[j];
            }
        } else {
            bf16_t* Cp = reinterpret_cast<bf16_t*>(d.C) + coff;
            if (full) {
                store4(Cp, v);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n + j < d.N) Cp[j] = f2bf(v[j]);
            }
        }
    }
    if (d.colsum) {      // the tile's column sums: over the wave's 8 rows in registers, over the 4 waves in LDS, one atomic per column
        const bool sq = d.colsumsq != nullptr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int o = 8; o < 64; o <<= 1) {
                cs[j] += __shfl_xor(cs[j], o, 64);
                cq[j] += __shfl_xor(cq[j], o, 64);
            }
        }
        __syncthreads();      // the partial tiles are read
        float* red = &part[0][0];      // [sum | sum of squares][wave][32 columns]
        if (lane < 8) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                red[wave * 32 + lane * 4 + j] = cs[j];
                red[128 + wave * 32 + lane * 4 + j] = cq[j];
            }
        }
        __syncthreads();
        if (tid < 64) {
            const int which = tid >> 5, col = tid & 31;
            if (n0 + col < d.N && (which == 0 || sq)) {
                const float* r = red + which * 128 + col;
                const float s = (r[0] + r[32]) + (r[64] + r[96]);
                atomicAdd((which ? d.colsumsq : d.colsum) + z * d.strideCol + n0 + col, s);
            }
        }
    }
}

// ================================================================================================
// TN, 64 x 64 tile, the whole reduction inside the workgroup
// ================================================================================================
constexpr int kFrTnRows = 128;       // reduction rows per LDS image
constexpr int kFrTnRowBytes = 256;   // 64 Y columns + 64 X columns

__device__ __forceinline__ int fr_tn_swz(int row) { return ((row & 3) << 1) | (((row >> 3) & 1) << 3); }      // gemm.hip: tn_swz

__global__ __launch_bounds__(kFrThreads) void gemm_tn_fewrows_kernel(const ga_wgrad_desc d) {
    __shared__ __attribute__((aligned(16))) unsigned char img[kFrTnRows * kFrTnRowBytes];      // 32 KiB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wk = wave & 1;      // 32 x 32 of the tile per wave
    const int tiles_k = (d.K + 63) >> 6;
    const int tile_n = blockIdx.x / tiles_k, tile_k = blockIdx.x - tile_n * tiles_k;
    const int n0 = tile_n * 64, k0 = tile_k * 64;
    const long z = blockIdx.z;
    const long zx = d.x_batch_mod > 0 ? z % d.x_batch_mod : z;
    const bf16_t* Yb = reinterpret_cast<const bf16_t*>(d.Y) + z * d.strideY;
    const bf16_t* Xb = reinterpret_cast<const bf16_t*>(d.X) + zx * d.strideX;

    // staging: thread = chunk column cc (0..7: Y, 8..15: X) of rows rr, rr + 16, ...
    const int cc = tid & 15, rr = tid >> 4;
    const bool is_y = cc < 8;
    const int col = is_y ? n0 + cc * 8 : k0 + (cc - 8) * 8;
    // N % 8 == 0; K may be ragged: ldx covers K rounded up to 8 (tn_validate), the columns past K meet only outputs that are not stored
    const bool col_ok = is_y ? col < d.N : col < d.K;
    const bf16_t* src = col_ok ? (is_y ? Yb + col : Xb + col) : Yb;
    const long ld = col_ok ? (is_y ? d.ldy : d.ldx) : d.ldy;
    const bool do_bias = d.dbias != nullptr && tile_k == 0;      // the column sums of Y: once, by the workgroups of one K tile
    uint4 rg[8];
    float bsum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bsum[j] = 0.f;

    auto g_load = [&](int slab) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const long m = (long)slab * kFrTnRows + rr + 16 * i;
            const uint4 t = *reinterpret_cast<const uint4*>(src + (m < d.M ? m : d.M - 1) * ld);
            rg[i] = (col_ok && m < d.M) ? t : fr_zero4();
        }
    };
    auto s_store = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = rr + 16 * i;
            *reinterpret_cast<uint4*>(img + row * kFrTnRowBytes + ((cc ^ fr_tn_swz(row)) << 4)) = rg[i];
            if (do_bias && is_y) {
                float y[8];
                unpack8(rg[i], y);
#pragma unroll
                for (int j = 0; j < 8; ++j) bsum[j] += y[j];
            }
        }
    };

    f32x4_t acc[2][2];      // [n block][k block]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nslabs = (d.M + kFrTnRows - 1) / kFrTnRows;
    g_load(0);
    for (int s = 0; s < nslabs; ++s) {
        s_store();
        __syncthreads();
        if (s + 1 < nslabs) g_load(s + 1);
        const int rows = min(kFrTnRows, d.M - s * kFrTnRows);
#pragma unroll
        for (int ks = 0; ks < kFrTnRows / 32; ++ks) {      // 32 reduction rows per MFMA
            if (ks * 32 >= rows) break;
            s16x4_t yf[2][2], xf[2][2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int row = ks * 32 + 8 * (lane >> 4) + 4 * hf + ((lane & 15) >> 2);
                const int sw = fr_tn_swz(row);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int ch_y = ((wn * 32 + t * 16) >> 3) + ((lane & 3) >> 1);
                    const int ch_x = 8 + ((wk * 32 + t * 16) >> 3) + ((lane & 3) >> 1);
                    const unsigned ay = row * kFrTnRowBytes + ((ch_y ^ sw) << 4) + 8 * (lane & 1);
                    const unsigned ax = row * kFrTnRowBytes + ((ch_x ^ sw) << 4) + 8 * (lane & 1);
                    yf[t][hf] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(img + ay));
                    xf[t][hf] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(img + ax));
                }
            }
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int tk = 0; tk < 2; ++tk)
                    acc[tn][tk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(&yf[tn][0]),
                                                                          *reinterpret_cast<const bf16x8_t*>(&xf[tk][0]),
                                                                          acc[tn][tk], 0, 0, 0);
        }
        __syncthreads();      // the image is read: the next rows may be stored
    }

    // ---- write out: D[n][k]; lane: k = lane & 15 (column), n = (lane >> 4) * 4 + r (rows).  One workgroup owns the tile: the
    // atomic of `accumulate` only keeps a concurrent launch into the same dW correct, as in gemm_tn_kernel
    float* W = d.dW + z * d.strideW;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tk = 0; tk < 2; ++tk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wn * 32 + tn * 16 + (lane >> 4) * 4 + r;
                const int k = k0 + wk * 32 + tk * 16 + (lane & 15);
                if (n < d.N && k < d.K) {
                    const float v = acc[tn][tk][r] * d.alpha;
                    if (d.accumulate) atomicAdd(W + (long)n * d.ldw + k, v);
                    else W[(long)n * d.ldw + k] = v;
                }
            }
    if (do_bias) {      // the per-thread column sums over the 16 row groups, in a fixed order
        float* red = reinterpret_cast<float*>(img);      // [16][64]
        if (is_y) {
#pragma unroll
            for (int j = 0; j < 8; ++j) red[rr * 64 + cc * 8 + j] = bsum[j];
        }
        __syncthreads();
        if (tid < 64 && n0 + tid < d.N) {
            float s = 0.f;
            for (int r = 0; r < 16; ++r) s += red[r * 64 + tid];
            atomicAdd(d.dbias + z * d.strideDbias + n0 + tid, s * d.alpha);
        }
    }
}

}  // namespace

extern "C" int ga_gemm_fewrows(const ga_gemm_desc* d, ga_stream_t stream) {
    if (const int rc = nt_validate(d)) return rc;
    if (!nt_fewrows_wanted(d, ga_num_cus(), current_knobs())) return ga_gemm(d, stream);
    dim3 grid(cdiv(d->M, 32) * cdiv(d->N, 32), 1, d->batch), block(kFrThreads);
    hipLaunchKernelGGL(gemm_nt_fewrows_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), *d);
    return ga_check_launch("ga_gemm_fewrows");
}

extern "C" int ga_gemm_fewrows_form(const ga_gemm_desc* d, char* buf, size_t n) {
    if (const int rc = nt_validate(d)) return rc;
    if (buf && n) nt_fewrows_name(d, nt_fewrows_wanted(d, ga_num_cus(), current_knobs()), buf, n);
    return GA_OK;
}

extern "C" int ga_wgrad_fewrows(const ga_wgrad_desc* d, ga_stream_t stream) {
    if (const int rc = tn_validate(d)) return rc;
    if (!tn_fewrows_wanted(d, ga_num_cus(), current_knobs())) return ga_wgrad(d, stream);
    dim3 grid(cdiv(d->N, 64) * cdiv(d->K, 64), 1, d->batch), block(kFrThreads);
    hipLaunchKernelGGL(gemm_tn_fewrows_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), *d);
    return ga_check_launch("ga_wgrad_fewrows");
}

extern "C" int ga_wgrad_fewrows_form(const ga_wgrad_desc* d, char* buf, size_t n) {
    if (const int rc = tn_validate(d)) return rc;
    if (buf && n) snprintf(buf, n, "%s", tn_fewrows_wanted(d, ga_num_cus(), current_knobs()) ? "fewrows_tn64x64" : "none");
    return GA_OK;
}
