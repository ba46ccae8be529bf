// The ResNet-only hot path of MAP-ResNet50 (MAP/models/map_resnet.py:21-80, 265-275) for gfx950: NHWC, C % 8 == 0, bf16 / fp32
// activations with fp32 math.  Every kernel is HBM-bound VALU work (no MFMA); threads own 8-channel chunks (16-byte loads in bf16).
//
//   maxpool3s2_fwd / _bwd ..... MaxPool2d(3, 2, 1): forward keeps a uint8 window index (0..8, row-major) per output element;
//                               backward is a gather (each input pixel sums the <= 2 x 2 outputs that chose it), no atomics
//   bn_gelu_fwd ............... y = gelu_erf(x * scale[c] + shift[c]) (ConvNormAct with nn.GELU, BatchNorm folded to scale / shift)
//   bn_gelu_bwd_reduce / _apply the BatchNorm backward through the GELU from the RAW conv output x (no stored pre-activation):
//                               g = dy * gelu'(x * scale + shift); reduce: s1 = sum g, s2 = sum g * xhat (per-workgroup partials
//                               in a caller workspace, then one ordered reduction); apply: dx = w * rstd * (g - s1/n - xhat s2/n)
//   se_bn_fwd / _bwd .......... SEUnit (:31-41) with a BatchNorm over the batch in its hidden layer, from the per-sample spatial sums
//                               of the RAW conv3 output: p = scale3 * sum / HW + shift3 is the pooled BatchNorm-3 output
//   se_residual_fwd ........... y = relu(res' + r[b] * gate[b][c] * (x3 * scale3 + shift3)), res' = res * rscale + rshift (or res)
//   se_residual_bwd_a / _b .... the backward of that tail and of BatchNorm 3 in two passes over the big tensors (see below)
//   subsample2_fwd / _bwd ..... the stride-2 input of the 1 x 1 / 2 downsample conv, and its zero-filling transpose
#include <algorithm>
#include <type_traits>
#include "common.h"

namespace {

constexpr int kThreads = 256;

int blocks_for(long items, int per_block = kThreads, int max_blocks = 4096) {
    return (int)std::max<long>(1, std::min<long>(max_blocks, (items + per_block - 1) / per_block));
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int unsupported(const char* who, long rows, int C) {
    if (rows <= 0 || C <= 0 || C % 8 != 0 || rows * (long)C >= (1L << 40)) {
        ga_set_error("%s: unsupported shape (rows %ld, C %d): C must be a positive multiple of 8", who, rows, C);
        return GA_ERR_UNSUPPORTED;
    }
    return GA_OK;
}

template <typename T> struct is_bf : std::false_type {};
template <> struct is_bf<bf16_t> : std::true_type {};

// ---------------------------------------------------------------------------------------------------------------------------
// MaxPool2d(3, stride 2, pad 1).  The window of output (oy, ox) is rows 2oy-1 .. 2oy+1, cols 2ox-1 .. 2ox+1 (clipped); PyTorch's
// rule: scan in row-major order, take a value when it is > the running maximum or NaN (so NaN propagates); the index starts at the
// first in-bounds tap.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, unsigned char* __restrict__ idx,
                                                               int H, int W, int C, int Ho, int Wo, long n8) {
    const int C8 = C / 8;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (long)gridDim.x * kThreads) {
        const int c = (int)(i % C8) * 8;
        const long p = i / C8;
        const int ox = (int)(p % Wo);
        const long r = p / Wo;
        const int oy = (int)(r % Ho), b = (int)(r / Ho);
        const int y0 = max(2 * oy - 1, 0), x0 = max(2 * ox - 1, 0);
        float best[8];
        int arg[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            best[j] = -INFINITY;
            arg[j] = (y0 - (2 * oy - 1)) * 3 + (x0 - (2 * ox - 1));
        }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
            if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                if ((unsigned)ix >= (unsigned)W) continue;
                float v[8];
                load8(x + (((long)b * H + iy) * W + ix) * C + c, v);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (v[j] > best[j] || v[j] != v[j]) {
                        best[j] = v[j];
                        arg[j] = ky * 3 + kx;
                    }
            }
        }
        store8(y + p * C + c, best);
        if (idx) {
            uint2 pk;
            pk.x = (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
            pk.y = (unsigned)arg[4] | ((unsigned)arg[5] << 8) | ((unsigned)arg[6] << 16) | ((unsigned)arg[7] << 24);
            *reinterpret_cast<uint2*>(idx + p * C + c) = pk;
        }
    }
}

// dx[b, iy, ix, c] (+)= sum over the outputs (oy, ox) whose window holds (iy, ix) at tap k = (iy-2oy+1)*3 + (ix-2ox+1) and whose
// saved index is k, of dy[b, oy, ox, c]; fixed order oy, ox ascending (deterministic)
template <typename T>
__global__ __launch_bounds__(kThreads) void maxpool_bwd_kernel(const T* __restrict__ dy, const unsigned char* __restrict__ idx, T* __restrict__ dx,
                                                               int H, int W, int C, int Ho, int Wo, long n8, int accumulate) {
    const int C8 = C / 8;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (long)gridDim.x * kThreads) {
        const int c = (int)(i % C8) * 8;
        const long p = i / C8;
        const int ix = (int)(p % W);
        const long r = p / W;
        const int iy = (int)(r % H), b = (int)(r / H);
        float acc[8];
        if (accumulate) load8(dx + p * C + c, acc);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        }
        // oy with 2oy-1 <= iy <= 2oy+1  ->  oy in [ceil((iy-1)/2), floor((iy+1)/2)]
        const int oy0 = iy / 2, oy1 = min((iy + 1) / 2, Ho - 1);
        const int ox0 = ix / 2, ox1 = min((ix + 1) / 2, Wo - 1);
        for (int oy = oy0; oy <= oy1; ++oy) {
            const int ky = iy - 2 * oy + 1;
            for (int ox = ox0; ox <= ox1; ++ox) {
                const int kx = ix - 2 * ox + 1;
                const long o = (((long)b * Ho + oy) * Wo + ox) * C + c;
                const uint2 pk = *reinterpret_cast<const uint2*>(idx + o);
                float g[8];
                load8(dy + o, g);
                const unsigned k = (unsigned)(ky * 3 + kx);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned a = ((j < 4 ? pk.x : pk.y) >> (8 * (j & 3))) & 0xffu;
                    if (a == k) acc[j] += g[j];
                }
            }
        }
        store8(dx + p * C + c, acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// BatchNorm-apply + GELU
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void bn_gelu_fwd_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, T* __restrict__ y, long n8, int C) {
    const int C8 = C / 8;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (long)gridDim.x * kThreads) {
        const int c = (int)(i % C8) * 8;
        float v[8];
        load8(x + i * 8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = gelu_f(fmaf(v[j], scale[c + j], shift[c + j]));
        store8(y + i * 8, v);
    }
}

// reduce: workgroup (gx, gy) owns channel chunks [gx * CPB, +CPB) and the rows gy, gy + gridDim.y, ...; thread = (row lane, chunk);
// its partial sums go through an ordered LDS reduction into part[gy][C] (s1) and part[gridDim.y + gy][C] (s2)
constexpr int kRedCPB = 8;                  // chunks per workgroup (64 channels)
constexpr int kRedPL = kThreads / kRedCPB;  // row lanes
constexpr int kRedGY = 256;                 // partial rows at most

template <typename T>
__global__ __launch_bounds__(kThreads) void bn_gelu_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                      float* __restrict__ part, long rows, int C) {
    __shared__ float red[2][kThreads * 8];
    const int t = threadIdx.x, cc = t % kRedCPB, pl = t / kRedCPB;
    const int chunk = blockIdx.x * kRedCPB + cc;
    const bool active = chunk < C / 8;
    const int c = chunk * 8;
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
    if (active) {
        float sc[8], sh[8], mu[8], rs[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sc[j] = scale[c + j];
            sh[j] = shift[c + j];
            mu[j] = mean[c + j];
            rs[j] = rstd[c + j];
        }
        for (long r = (long)blockIdx.y * kRedPL + pl; r < rows; r += (long)gridDim.y * kRedPL) {
            float g[8], xv[8];
            load8(dy + r * C + c, g);
            load8(x + r * C + c, xv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float gg = g[j] * gelu_grad_f(fmaf(xv[j], sc[j], sh[j]));
                s1[j] += gg;
                s2[j] = fmaf(gg, (xv[j] - mu[j]) * rs[j], s2[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        red[0][t * 8 + j] = s1[j];
        red[1][t * 8 + j] = s2[j];
    }
    __syncthreads();
    const int ch0 = blockIdx.x * kRedCPB * 8;
    for (int v = t; v < 2 * kRedCPB * 8; v += kThreads) {
        const int which = v / (kRedCPB * 8), rr = v % (kRedCPB * 8);
        float s = 0.f;
        for (int p = 0; p < kRedPL; ++p) s += red[which][p * kRedCPB * 8 + rr];
        if (ch0 + rr < C) part[((long)which * gridDim.y + blockIdx.y) * C + ch0 + rr] = s;
    }
}

// out[c] = sum over gy (ascending) of part[gy][c]; s1 from the first half, s2 from the second
__global__ __launch_bounds__(kThreads) void partial_sum_kernel(const float* __restrict__ part, float* __restrict__ s1, float* __restrict__ s2,
                                                               int gy, int C) {
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= 2 * C) return;
    const int which = v / C, c = v % C;
    const float* p = part + (long)which * gy * C + c;
    float s = 0.f;
    for (int k = 0; k < gy; ++k) s += p[(long)k * C];
    (which ? s2 : s1)[c] = s;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void bn_gelu_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                     const float* __restrict__ scale, const float* __restrict__ shift,
                                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                     const float* __restrict__ w, const float* __restrict__ s1,
                                                                     const float* __restrict__ s2, float inv_n, T* __restrict__ dx,
                                                                     long n8, int C) {
    const int C8 = C / 8;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (long)gridDim.x * kThreads) {
        const int c = (int)(i % C8) * 8;
        float g[8], xv[8];
        load8(dy + i * 8, g);
        load8(x + i * 8, xv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int cj = c + j;
            const float rs = rstd[cj];
            const float gg = g[j] * gelu_grad_f(fmaf(xv[j], scale[cj], shift[cj]));
            const float xh = (xv[j] - mean[cj]) * rs;
            g[j] = (w ? w[cj] : 1.f) * rs * (gg - s1[cj] * inv_n - xh * s2[cj] * inv_n);
        }
        store8(dx + i * 8, g);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// SE unit with BatchNorm over the batch.  Layout: S [B][C] = sum_hw of the raw conv3 output (fp32), p = scale3 * S / HW + shift3;
// W1 [R][C] (no bias), BatchNorm (g1, b1) over the B rows, GELU, W2 [C][R] + b2, sigmoid.
//   fwd1: one workgroup per hidden unit r: hpre[:, r] (one wave per sample row), its batch statistics (train) or the running ones
//         (eval), h = gelu(bn(hpre)); the running-stat update (momentum 0.1, unbiased variance) is the workgroup's own
//   fwd2: gate[b][c] = sigmoid(b2[c] + sum_r h[b][r] W2[c][r]); a workgroup = 8 sample rows (in LDS) x 256 channels
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kSeRows = 8;
constexpr int kSeMaxB = 1024, kSeMaxC = 2048, kSeMaxR = 128;

__device__ __forceinline__ float block_sum(float v, float* sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    float s = 0.f;
    for (int k = 0; k < kThreads / 64; ++k) s += sh[k];
    return s;
}

__global__ __launch_bounds__(kThreads) void se_fwd1_kernel(const float* __restrict__ S, float inv_hw, const float* __restrict__ scale3,
                                                           const float* __restrict__ shift3, const float* __restrict__ W1,
                                                           const float* __restrict__ g1, const float* __restrict__ b1,
                                                           float* __restrict__ rmean, float* __restrict__ rvar, float* __restrict__ hpre,
                                                           float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ h,
                                                           int B, int C, int R, int training) {
    __shared__ float hp[kSeMaxB];
    __shared__ float sh[kThreads / 64];
    const int r = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* w = W1 + (long)r * C;
    for (int b = wv; b < B; b += kThreads / 64) {
        const float* s = S + (long)b * C;
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc = fmaf(w[c], fmaf(scale3[c], s[c] * inv_hw, shift3[c]), acc);
        acc = wave_sum(acc);
        if (lane == 0) hp[b] = acc;
    }
    __syncthreads();
    float mu, rs;
    if (training) {
        float a = 0.f;
        for (int b = threadIdx.x; b < B; b += kThreads) a += hp[b];
        mu = block_sum(a, sh) / (float)B;
        float q = 0.f;
        for (int b = threadIdx.x; b < B; b += kThreads) q += (hp[b] - mu) * (hp[b] - mu);
        const float var = block_sum(q, sh) / (float)B;
        rs = rsqrtf(var + 1e-5f);
        if (threadIdx.x == 0) {
            rmean[r] = 0.9f * rmean[r] + 0.1f * mu;
            rvar[r] = 0.9f * rvar[r] + 0.1f * var * (float)B / (float)(B - 1);
        }
    } else {
        mu = rmean[r];
        rs = rsqrtf(rvar[r] + 1e-5f);
    }
    if (threadIdx.x == 0) {
        mean[r] = mu;
        rstd[r] = rs;
    }
    const float a = g1[r] * rs, sft = b1[r] - mu * a;
    for (int b = threadIdx.x; b < B; b += kThreads) {
        hpre[(long)b * R + r] = hp[b];
        h[(long)b * R + r] = gelu_f(fmaf(hp[b], a, sft));
    }
}

__global__ __launch_bounds__(kThreads) void se_fwd2_kernel(const float* __restrict__ h, const float* __restrict__ W2,
                                                           const float* __restrict__ b2, float* __restrict__ gate, int B, int C, int R) {
    __shared__ float hs[kSeRows][kSeMaxR];
    const int b0 = blockIdx.y * kSeRows;
    for (int v = threadIdx.x; v < kSeRows * R; v += kThreads) {
        const int bb = v / R, rr = v % R;
        hs[bb][rr] = b0 + bb < B ? h[(long)(b0 + bb) * R + rr] : 0.f;
    }
    __syncthreads();
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    float acc[kSeRows];
#pragma unroll
    for (int bb = 0; bb < kSeRows; ++bb) acc[bb] = b2[c];
    const float* w = W2 + (long)c * R;
    for (int rr = 0; rr < R; ++rr) {
        const float wv = w[rr];
#pragma unroll
        for (int bb = 0; bb < kSeRows; ++bb) acc[bb] = fmaf(hs[bb][rr], wv, acc[bb]);
    }
#pragma unroll
    for (int bb = 0; bb < kSeRows; ++bb)
        if (b0 + bb < B) gate[(long)(b0 + bb) * C + c] = 1.f / (1.f + __expf(-acc[bb]));
}

// SE backward.  Inputs from the tail's pass A: P1 = sum_hw dm, P2 = sum_hw dm * xhat3 (per (b, c)), with dm the gradient of the
// block's pre-ReLU sum; dgate = r * (g3 P2 + b3 P1).
//   bwd1: dz = dgate * gate * (1 - gate)                                                          ([B][C], elementwise)
//   bwd2: one workgroup per hidden unit r: dh = sum_c dz W2[c][r], GELU' and the BatchNorm backward over the batch -> dhpre[:, r],
//         dg1[r], db1[r]; then its rows of dW1 (sum_b dhpre p) and its column of dW2 (sum_b dz h)       (+=, one owner each)
//   bwd3: ds[b][c] = sum_r dhpre[b][r] W1[r][c]: the gradient of the pooled BatchNorm-3 output p     (8 rows x 256 channels)
//   bwd4: per channel, over b in order: db2 += sum dz; the BatchNorm-3 sums of du = dm g r + ds / HW:
//         s1 = sum_b (g r P1 + ds), s2 = sum_b (g r P2 + ds / HW * sum_hw xhat3), sum_hw xhat3 = rstd3 (S - HW mean3)
__global__ __launch_bounds__(kThreads) void se_bwd1_kernel(const float* __restrict__ P1, const float* __restrict__ P2,
                                                           const float* __restrict__ rowscale, const float* __restrict__ g3,
                                                           const float* __restrict__ b3, const float* __restrict__ gate,
                                                           float* __restrict__ dz, int B, int C) {
    const long n = (long)B * C;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        const int c = (int)(i % C), b = (int)(i / C);
        const float r = rowscale ? rowscale[b] : 1.f;
        const float dg = r * fmaf(g3[c], P2[i], b3[c] * P1[i]);
        const float g = gate[i];
        dz[i] = dg * g * (1.f - g);
    }
}

__global__ __launch_bounds__(kThreads) void se_bwd2_kernel(const float* __restrict__ dz, const float* __restrict__ S, float inv_hw,
                                                           const float* __restrict__ scale3, const float* __restrict__ shift3,
                                                           const float* __restrict__ W2, const float* __restrict__ g1,
                                                           const float* __restrict__ b1, const float* __restrict__ hpre,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ h, float* __restrict__ dhpre, float* __restrict__ dW1,
                                                           float* __restrict__ dg1, float* __restrict__ db1, float* __restrict__ dW2,
                                                           int B, int C, int R) {
    __shared__ float g[kSeMaxB], xh[kSeMaxB], hv[kSeMaxB];
    __shared__ float sh[kThreads / 64];
    const int r = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float mu = mean[r], rs = rstd[r], ga = g1[r], be = b1[r];
    for (int b = wv; b < B; b += kThreads / 64) {
        const float* d = dz + (long)b * C;
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc = fmaf(d[c], W2[(long)c * R + r], acc);
        acc = wave_sum(acc);
        if (lane == 0) {
            const float x = (hpre[(long)b * R + r] - mu) * rs;
            g[b] = acc * gelu_grad_f(fmaf(x, ga, be));
            xh[b] = x;
            hv[b] = h[(long)b * R + r];
        }
    }
    __syncthreads();
    float a1 = 0.f, a2 = 0.f;
    for (int b = threadIdx.x; b < B; b += kThreads) {
        a1 += g[b];
        a2 = fmaf(g[b], xh[b], a2);
    }
    const float t1 = block_sum(a1, sh);
    const float t2 = block_sum(a2, sh);
    if (threadIdx.x == 0) {
        db1[r] += t1;
        dg1[r] += t2;
    }
    const float inv_b = 1.f / (float)B, A = ga * rs;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += kThreads) {
        const float d = A * (g[b] - t1 * inv_b - xh[b] * t2 * inv_b);
        g[b] = d;
        dhpre[(long)b * R + r] = d;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += kThreads) {
        const float sc = scale3[c] * inv_hw, sf = shift3[c];
        float w1 = 0.f, w2 = 0.f;
        for (int b = 0; b < B; ++b) {
            w1 = fmaf(g[b], fmaf(sc, S[(long)b * C + c], sf), w1);
            w2 = fmaf(dz[(long)b * C + c], hv[b], w2);
        }
        dW1[(long)r * C + c] += w1;
        dW2[(long)c * R + r] += w2;
    }
}

__global__ __launch_bounds__(kThreads) void se_bwd3_kernel(const float* __restrict__ dhpre, const float* __restrict__ W1,
                                                           float* __restrict__ ds, int B, int C, int R) {
    __shared__ float hs[kSeRows][kSeMaxR];
    const int b0 = blockIdx.y * kSeRows;
    for (int v = threadIdx.x; v < kSeRows * R; v += kThreads) {
        const int bb = v / R, rr = v % R;
        hs[bb][rr] = b0 + bb < B ? dhpre[(long)(b0 + bb) * R + rr] : 0.f;
    }
    __syncthreads();
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    float acc[kSeRows];
#pragma unroll
    for (int bb = 0; bb < kSeRows; ++bb) acc[bb] = 0.f;
    for (int rr = 0; rr < R; ++rr) {
        const float wv = W1[(long)rr * C + c];
#pragma unroll
        for (int bb = 0; bb < kSeRows; ++bb) acc[bb] = fmaf(hs[bb][rr], wv, acc[bb]);
    }
#pragma unroll
    for (int bb = 0; bb < kSeRows; ++bb)
        if (b0 + bb < B) ds[(long)(b0 + bb) * C + c] = acc[bb];
}

__global__ __launch_bounds__(kThreads) void se_bwd4_kernel(const float* __restrict__ P1, const float* __restrict__ P2,
                                                           const float* __restrict__ rowscale, const float* __restrict__ gate,
                                                           const float* __restrict__ dz, const float* __restrict__ ds,
                                                           const float* __restrict__ S, const float* __restrict__ mean3,
                                                           const float* __restrict__ rstd3, float* __restrict__ s1, float* __restrict__ s2,
                                                           float* __restrict__ db2, int B, int C, int HW) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    const float inv_hw = 1.f / (float)HW, mu = mean3[c], rs = rstd3[c];
    float a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int b = 0; b < B; ++b) {
        const long i = (long)b * C + c;
        const float gr = gate[i] * (rowscale ? rowscale[b] : 1.f);
        const float d = ds[i];
        a1 += fmaf(gr, P1[i], d);
        a2 += fmaf(gr, P2[i], d * inv_hw * rs * (S[i] - (float)HW * mu));
        a3 += dz[i];
    }
    s1[c] = a1;
    s2[c] = a2;
    db2[c] += a3;
}

// ---------------------------------------------------------------------------------------------------------------------------
// SE-scale + DropPath + residual + ReLU
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void se_res_fwd_kernel(const T* __restrict__ x3, const float* __restrict__ scale3,
                                                              const float* __restrict__ shift3, const float* __restrict__ gate,
                                                              const float* __restrict__ rowscale, const T* __restrict__ res,
                                                              const float* __restrict__ rscale, const float* __restrict__ rshift,
                                                              T* __restrict__ y, long n8, int HW, int C) {
    const int C8 = C / 8;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (long)gridDim.x * kThreads) {
        const int c = (int)(i % C8) * 8;
        const int b = (int)(i / ((long)C8 * HW));
        const float r = rowscale ? rowscale[b] : 1.f;
        const float* gt = gate + (long)b * C + c;
        float xv[8], rv[8];
        load8(x3 + i * 8, xv);
        load8(res + i * 8, rv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float rr = rscale ? fmaf(rv[j], rscale[c + j], rshift[c + j]) : rv[j];
            xv[j] = fmaxf(fmaf(r * gt[j], fmaf(xv[j], scale3[c + j], shift3[c + j]), rr), 0.f);
        }
        store8(y + i * 8, xv);
    }
}

// pass A: workgroup (gx, b) owns channel chunks [gx * kACPB, +kACPB) of sample b over all HW pixels; dm = dy * (y > 0) is written,
// P1 = sum_hw dm and P2 = sum_hw dm * xhat3 reduced in order over the pixel lanes (no atomics)
constexpr int kACPB = 8;
constexpr int kAPL = kThreads / kACPB;

template <typename T>
__global__ __launch_bounds__(kThreads) void se_res_bwd_a_kernel(const T* __restrict__ dy, const T* __restrict__ y, const T* __restrict__ x3,
                                                                const float* __restrict__ mean3, const float* __restrict__ rstd3,
                                                                T* __restrict__ dm, float* __restrict__ P1, float* __restrict__ P2,
                                                                int HW, int C) {
    __shared__ float red[2][kThreads * 8];
    const int t = threadIdx.x, cc = t % kACPB, pl = t / kACPB;
    const int chunk = blockIdx.x * kACPB + cc;
    const bool active = chunk < C / 8;
    const int c = chunk * 8, b = blockIdx.y;
    float a1[8], a2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a1[j] = a2[j] = 0.f;
    if (active) {
        float mu[8], rs[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            mu[j] = mean3[c + j];
            rs[j] = rstd3[c + j];
        }
        for (int p = pl; p < HW; p += kAPL) {
            const long e = ((long)b * HW + p) * C + c;
            float g[8], yv[8], xv[8];
            load8(dy + e, g);
            load8(y + e, yv);
            load8(x3 + e, xv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                g[j] = yv[j] > 0.f ? g[j] : 0.f;
                if (is_bf<T>::value) g[j] = elt<T>::round(g[j]);      // the sums see the dm that is stored
                a1[j] += g[j];
                a2[j] = fmaf(g[j], (xv[j] - mu[j]) * rs[j], a2[j]);
            }
            store8(dm + e, g);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        red[0][t * 8 + j] = a1[j];
        red[1][t * 8 + j] = a2[j];
    }
    __syncthreads();
    const int ch0 = blockIdx.x * kACPB * 8;
    for (int v = t; v < 2 * kACPB * 8; v += kThreads) {
        const int which = v / (kACPB * 8), rr = v % (kACPB * 8);
        float s = 0.f;
        for (int p = 0; p < kAPL; ++p) s += red[which][p * kACPB * 8 + rr];
        if (ch0 + rr < C) (which ? P2 : P1)[(long)b * C + ch0 + rr] = s;
    }
}

// pass B: dx3 = g3 * rstd3 * (du - s1/n - xhat3 * s2/n), du = dm * gate * r + ds / HW
template <typename T>
__global__ __launch_bounds__(kThreads) void se_res_bwd_b_kernel(const T* __restrict__ dm, const T* __restrict__ x3,
                                                                const float* __restrict__ mean3, const float* __restrict__ rstd3,
                                                                const float* __restrict__ g3, const float* __restrict__ gate,
                                                                const float* __restrict__ rowscale, const float* __restrict__ ds,
                                                                const float* __restrict__ s1, const float* __restrict__ s2, float inv_n,
                                                                T* __restrict__ dx3, long n8, int HW, int C) {
    const int C8 = C / 8;
    const float inv_hw = 1.f / (float)HW;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (long)gridDim.x * kThreads) {
        const int c = (int)(i % C8) * 8;
        const int b = (int)(i / ((long)C8 * HW));
        const float r = rowscale ? rowscale[b] : 1.f;
        const float* gt = gate + (long)b * C + c;
        const float* d = ds + (long)b * C + c;
        float mv[8], xv[8];
        load8(dm + i * 8, mv);
        load8(x3 + i * 8, xv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int cj = c + j;
            const float rs = rstd3[cj];
            const float du = fmaf(mv[j], gt[j] * r, d[j] * inv_hw);
            const float xh = (xv[j] - mean3[cj]) * rs;
            mv[j] = g3[cj] * rs * (du - s1[cj] * inv_n - xh * s2[cj] * inv_n);
        }
        store8(dx3 + i * 8, mv);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// stride-2 subsample (the input of a 1 x 1 / 2 conv) and its transpose
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void subsample2_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int H, int W, int C, int Ho,
                                                                  int Wo, long n8) {
    const int C8 = C / 8;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (long)gridDim.x * kThreads) {
        const int c = (int)(i % C8) * 8;
        const long p = i / C8;
        const int ox = (int)(p % Wo);
        const long r = p / Wo;
        const int oy = (int)(r % Ho), b = (int)(r / Ho);
        float v[8];
        load8(x + (((long)b * H + 2 * oy) * W + 2 * ox) * C + c, v);
        store8(y + p * C + c, v);
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void subsample2_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int H, int W, int C, int Ho,
                                                                  int Wo, long n8, int accumulate) {
    const int C8 = C / 8;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (long)gridDim.x * kThreads) {
        const int c = (int)(i % C8) * 8;
        const long p = i / C8;
        const int ix = (int)(p % W);
        const long r = p / W;
        const int iy = (int)(r % H), b = (int)(r / H);
        const bool hit = !(iy & 1) && !(ix & 1);
        if (accumulate && !hit) continue;
        float v[8];
        if (hit) {
            load8(dy + (((long)b * Ho + iy / 2) * Wo + ix / 2) * C + c, v);
            if (accumulate) {
                float a[8];
                load8(dx + p * C + c, a);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] += a[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;
        }
        store8(dx + p * C + c, v);
    }
}

template <typename P> auto cp(const void* p) { return reinterpret_cast<const P*>(p); }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------
extern "C" int ga_maxpool3s2_fwd(const void* x, void* y, unsigned char* idx, int B, int H, int W, int C, int dtype, ga_stream_t stream) {
    GA_REQUIRE(x && y && (dtype == GA_BF16 || dtype == GA_F32) && B > 0 && H > 0 && W > 0, "ga_maxpool3s2_fwd: bad args");
    if (int e = unsupported("ga_maxpool3s2_fwd", (long)B * H * W, C)) return e;
    GA_REQUIRE(al16(x) && al16(y) && (reinterpret_cast<uintptr_t>(idx) & 7) == 0, "ga_maxpool3s2_fwd: x, y 16-byte, idx 8-byte aligned");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long n8 = (long)B * Ho * Wo * (C / 8);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16)
        hipLaunchKernelGGL(maxpool_fwd_kernel<bf16_t>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<bf16_t>(x), (bf16_t*)y, idx, H, W, C, Ho,
                           Wo, n8);
    else
        hipLaunchKernelGGL(maxpool_fwd_kernel<float>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<float>(x), (float*)y, idx, H, W, C, Ho,
                           Wo, n8);
    return ga_check_launch("ga_maxpool3s2_fwd");
}

extern "C" int ga_maxpool3s2_bwd(const void* dy, const unsigned char* idx, void* dx, int B, int H, int W, int C, int accumulate, int dtype,
                                 ga_stream_t stream) {
    GA_REQUIRE(dy && idx && dx && (dtype == GA_BF16 || dtype == GA_F32) && B > 0 && H > 0 && W > 0, "ga_maxpool3s2_bwd: bad args");
    if (int e = unsupported("ga_maxpool3s2_bwd", (long)B * H * W, C)) return e;
    GA_REQUIRE(al16(dy) && al16(dx) && (reinterpret_cast<uintptr_t>(idx) & 7) == 0, "ga_maxpool3s2_bwd: dy, dx 16-byte, idx 8-byte aligned");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long n8 = (long)B * H * W * (C / 8);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16)
        hipLaunchKernelGGL(maxpool_bwd_kernel<bf16_t>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<bf16_t>(dy), idx, (bf16_t*)dx, H, W, C,
                           Ho, Wo, n8, accumulate);
    else
        hipLaunchKernelGGL(maxpool_bwd_kernel<float>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<float>(dy), idx, (float*)dx, H, W, C,
                           Ho, Wo, n8, accumulate);
    return ga_check_launch("ga_maxpool3s2_bwd");
}

extern "C" int ga_bn_gelu_fwd(const void* x, const float* scale, const float* shift, void* y, int64_t rows, int C, int dtype,
                              ga_stream_t stream) {
    GA_REQUIRE(x && scale && shift && y && (dtype == GA_BF16 || dtype == GA_F32), "ga_bn_gelu_fwd: bad args");
    if (int e = unsupported("ga_bn_gelu_fwd", rows, C)) return e;
    GA_REQUIRE(al16(x) && al16(y), "ga_bn_gelu_fwd: x and y must be 16-byte aligned");
    const long n8 = rows * C / 8;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16)
        hipLaunchKernelGGL(bn_gelu_fwd_kernel<bf16_t>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<bf16_t>(x), scale, shift, (bf16_t*)y, n8, C);
    else
        hipLaunchKernelGGL(bn_gelu_fwd_kernel<float>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<float>(x), scale, shift, (float*)y, n8, C);
    return ga_check_launch("ga_bn_gelu_fwd");
}

namespace {
int red_gy(long rows, int C) {
    const int gx = (C / 8 + kRedCPB - 1) / kRedCPB;
    return (int)std::max<long>(1, std::min<long>({(long)kRedGY, (rows + kRedPL - 1) / kRedPL, std::max(1L, 2048L / gx)}));
}
}  // namespace

extern "C" size_t ga_bn_gelu_bwd_workspace(int64_t rows, int C) {
    if (rows <= 0 || C <= 0 || C % 8 != 0) return 0;
    return (size_t)2 * red_gy(rows, C) * C * sizeof(float);
}

extern "C" int ga_bn_gelu_bwd_reduce(const void* dy, const void* x, const float* scale, const float* shift, const float* mean,
                                     const float* rstd, float* s1, float* s2, int64_t rows, int C, int dtype, void* workspace,
                                     size_t ws_bytes, ga_stream_t stream) {
    GA_REQUIRE(dy && x && scale && shift && mean && rstd && s1 && s2 && (dtype == GA_BF16 || dtype == GA_F32),
               "ga_bn_gelu_bwd_reduce: bad args");
    if (int e = unsupported("ga_bn_gelu_bwd_reduce", rows, C)) return e;
    GA_REQUIRE(al16(dy) && al16(x), "ga_bn_gelu_bwd_reduce: dy and x must be 16-byte aligned");
    const size_t need = ga_bn_gelu_bwd_workspace(rows, C);
    GA_REQUIRE(workspace && ws_bytes >= need, "ga_bn_gelu_bwd_reduce: needs %zu B of workspace (ga_bn_gelu_bwd_workspace)", need);
    const int gx = (C / 8 + kRedCPB - 1) / kRedCPB, gy = red_gy(rows, C);
    float* part = static_cast<float*>(workspace);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16)
        hipLaunchKernelGGL(bn_gelu_bwd_reduce_kernel<bf16_t>, dim3(gx, gy), dim3(kThreads), 0, s, cp<bf16_t>(dy), cp<bf16_t>(x), scale, shift,
                           mean, rstd, part, (long)rows, C);
    else
        hipLaunchKernelGGL(bn_gelu_bwd_reduce_kernel<float>, dim3(gx, gy), dim3(kThreads), 0, s, cp<float>(dy), cp<float>(x), scale, shift,
                           mean, rstd, part, (long)rows, C);
    if (int e = ga_check_launch("ga_bn_gelu_bwd_reduce")) return e;
    hipLaunchKernelGGL(partial_sum_kernel, dim3(blocks_for(2L * C)), dim3(kThreads), 0, s, part, s1, s2, gy, C);
    return ga_check_launch("ga_bn_gelu_bwd_reduce.sum");
}

extern "C" int ga_bn_gelu_bwd_apply(const void* dy, const void* x, const float* scale, const float* shift, const float* mean,
                                    const float* rstd, const float* w, const float* s1, const float* s2, int64_t n, void* dx,
                                    int64_t rows, int C, int dtype, ga_stream_t stream) {
    GA_REQUIRE(dy && x && scale && shift && mean && rstd && s1 && s2 && dx && n > 0 && (dtype == GA_BF16 || dtype == GA_F32),
               "ga_bn_gelu_bwd_apply: bad args");
    if (int e = unsupported("ga_bn_gelu_bwd_apply", rows, C)) return e;
    GA_REQUIRE(al16(dy) && al16(x) && al16(dx), "ga_bn_gelu_bwd_apply: dy, x and dx must be 16-byte aligned");
    const long n8 = rows * C / 8;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16)
        hipLaunchKernelGGL(bn_gelu_bwd_apply_kernel<bf16_t>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<bf16_t>(dy), cp<bf16_t>(x), scale,
                           shift, mean, rstd, w, s1, s2, 1.f / (float)n, (bf16_t*)dx, n8, C);
    else
        hipLaunchKernelGGL(bn_gelu_bwd_apply_kernel<float>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<float>(dy), cp<float>(x), scale,
                           shift, mean, rstd, w, s1, s2, 1.f / (float)n, (float*)dx, n8, C);
    return ga_check_launch("ga_bn_gelu_bwd_apply");
}

namespace {
int se_check(const char* who, int B, int C, int R, int training) {
    if (B <= 0 || B > kSeMaxB || C <= 0 || C > kSeMaxC || C % 8 != 0 || R <= 0 || R > kSeMaxR || (training && B < 2)) {
        ga_set_error("%s: unsupported shape (B %d, C %d, R %d): B <= %d (>= 2 in train mode), C <= %d and C %% 8 == 0, R <= %d", who, B, C,
                     R, kSeMaxB, kSeMaxC, kSeMaxR);
        return GA_ERR_UNSUPPORTED;
    }
    return GA_OK;
}
}  // namespace

extern "C" int ga_se_bn_fwd(const float* S, int HW, const float* scale3, const float* shift3, const float* W1, const float* g1,
                            const float* b1, float* rmean, float* rvar, const float* W2, const float* b2, float* hpre, float* mean,
                            float* rstd, float* h, float* gate, int B, int C, int R, int training, ga_stream_t stream) {
    GA_REQUIRE(S && scale3 && shift3 && W1 && g1 && b1 && rmean && rvar && W2 && b2 && hpre && mean && rstd && h && gate && HW > 0,
               "ga_se_bn_fwd: bad args");
    if (int e = se_check("ga_se_bn_fwd", B, C, R, training)) return e;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(se_fwd1_kernel, dim3(R), dim3(kThreads), 0, s, S, 1.f / (float)HW, scale3, shift3, W1, g1, b1, rmean, rvar, hpre, mean,
                       rstd, h, B, C, R, training);
    if (int e = ga_check_launch("ga_se_bn_fwd.hidden")) return e;
    hipLaunchKernelGGL(se_fwd2_kernel, dim3((C + kThreads - 1) / kThreads, (B + kSeRows - 1) / kSeRows), dim3(kThreads), 0, s, h, W2, b2, gate,
                       B, C, R);
    return ga_check_launch("ga_se_bn_fwd.gate");
}

extern "C" int ga_se_bn_bwd(const float* P1, const float* P2, const float* rowscale, const float* g3, const float* b3, const float* mean3,
                            const float* rstd3, const float* S, int HW, const float* scale3, const float* shift3, const float* W1,
                            const float* g1, const float* b1, const float* W2, const float* hpre, const float* mean, const float* rstd,
                            const float* h, const float* gate, float* dz, float* dhpre, float* ds, float* s1, float* s2, float* dW1,
                            float* dg1, float* db1, float* dW2, float* db2, int B, int C, int R, ga_stream_t stream) {
    GA_REQUIRE(P1 && P2 && g3 && b3 && mean3 && rstd3 && S && scale3 && shift3 && W1 && g1 && b1 && W2 && hpre && mean && rstd && h &&
                   gate && dz && dhpre && ds && s1 && s2 && dW1 && dg1 && db1 && dW2 && db2 && HW > 0,
               "ga_se_bn_bwd: bad args");
    if (int e = se_check("ga_se_bn_bwd", B, C, R, 1)) return e;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(se_bwd1_kernel, dim3(blocks_for((long)B * C)), dim3(kThreads), 0, s, P1, P2, rowscale, g3, b3, gate, dz, B, C);
    if (int e = ga_check_launch("ga_se_bn_bwd.gate")) return e;
    hipLaunchKernelGGL(se_bwd2_kernel, dim3(R), dim3(kThreads), 0, s, dz, S, 1.f / (float)HW, scale3, shift3, W2, g1, b1, hpre, mean, rstd, h,
                       dhpre, dW1, dg1, db1, dW2, B, C, R);
    if (int e = ga_check_launch("ga_se_bn_bwd.hidden")) return e;
    hipLaunchKernelGGL(se_bwd3_kernel, dim3((C + kThreads - 1) / kThreads, (B + kSeRows - 1) / kSeRows), dim3(kThreads), 0, s, dhpre, W1, ds,
                       B, C, R);
    if (int e = ga_check_launch("ga_se_bn_bwd.pool")) return e;
    hipLaunchKernelGGL(se_bwd4_kernel, dim3((C + kThreads - 1) / kThreads), dim3(kThreads), 0, s, P1, P2, rowscale, gate, dz, ds, S, mean3,
                       rstd3, s1, s2, db2, B, C, HW);
    return ga_check_launch("ga_se_bn_bwd.sums");
}

extern "C" int ga_se_residual_fwd(const void* x3, const float* scale3, const float* shift3, const float* gate, const float* rowscale,
                                  const void* res, const float* rscale, const float* rshift, void* y, int B, int HW, int C, int dtype,
                                  ga_stream_t stream) {
    GA_REQUIRE(x3 && scale3 && shift3 && gate && res && y && (rscale == nullptr) == (rshift == nullptr) && B > 0 && HW > 0 &&
                   (dtype == GA_BF16 || dtype == GA_F32),
               "ga_se_residual_fwd: bad args (rscale and rshift go together)");
    if (int e = unsupported("ga_se_residual_fwd", (long)B * HW, C)) return e;
    GA_REQUIRE(al16(x3) && al16(res) && al16(y), "ga_se_residual_fwd: x3, res and y must be 16-byte aligned");
    const long n8 = (long)B * HW * C / 8;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16)
        hipLaunchKernelGGL(se_res_fwd_kernel<bf16_t>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<bf16_t>(x3), scale3, shift3, gate, rowscale,
                           cp<bf16_t>(res), rscale, rshift, (bf16_t*)y, n8, HW, C);
    else
        hipLaunchKernelGGL(se_res_fwd_kernel<float>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<float>(x3), scale3, shift3, gate, rowscale,
                           cp<float>(res), rscale, rshift, (float*)y, n8, HW, C);
    return ga_check_launch("ga_se_residual_fwd");
}

extern "C" int ga_se_residual_bwd_a(const void* dy, const void* y, const void* x3, const float* mean3, const float* rstd3, void* dm,
                                    float* P1, float* P2, int B, int HW, int C, int dtype, ga_stream_t stream) {
    GA_REQUIRE(dy && y && x3 && mean3 && rstd3 && dm && P1 && P2 && B > 0 && B < 65536 && HW > 0 && (dtype == GA_BF16 || dtype == GA_F32),
               "ga_se_residual_bwd_a: bad args");
    if (int e = unsupported("ga_se_residual_bwd_a", (long)B * HW, C)) return e;
    GA_REQUIRE(al16(dy) && al16(y) && al16(x3) && al16(dm), "ga_se_residual_bwd_a: dy, y, x3 and dm must be 16-byte aligned");
    const dim3 grid((C / 8 + kACPB - 1) / kACPB, B);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16)
        hipLaunchKernelGGL(se_res_bwd_a_kernel<bf16_t>, grid, dim3(kThreads), 0, s, cp<bf16_t>(dy), cp<bf16_t>(y), cp<bf16_t>(x3), mean3, rstd3,
                           (bf16_t*)dm, P1, P2, HW, C);
    else
        hipLaunchKernelGGL(se_res_bwd_a_kernel<float>, grid, dim3(kThreads), 0, s, cp<float>(dy), cp<float>(y), cp<float>(x3), mean3, rstd3,
                           (float*)dm, P1, P2, HW, C);
    return ga_check_launch("ga_se_residual_bwd_a");
}

extern "C" int ga_se_residual_bwd_b(const void* dm, const void* x3, const float* mean3, const float* rstd3, const float* g3, const float* gate,
                                    const float* rowscale, const float* ds, const float* s1, const float* s2, void* dx3, int B, int HW, int C,
                                    int dtype, ga_stream_t stream) {
    GA_REQUIRE(dm && x3 && mean3 && rstd3 && g3 && gate && ds && s1 && s2 && dx3 && B > 0 && HW > 0 && (dtype == GA_BF16 || dtype == GA_F32),
               "ga_se_residual_bwd_b: bad args");
    if (int e = unsupported("ga_se_residual_bwd_b", (long)B * HW, C)) return e;
    GA_REQUIRE(al16(dm) && al16(x3) && al16(dx3), "ga_se_residual_bwd_b: dm, x3 and dx3 must be 16-byte aligned");
    const long n8 = (long)B * HW * C / 8;
    const float inv_n = 1.f / (float)((long)B * HW);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16)
        hipLaunchKernelGGL(se_res_bwd_b_kernel<bf16_t>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<bf16_t>(dm), cp<bf16_t>(x3), mean3, rstd3,
                           g3, gate, rowscale, ds, s1, s2, inv_n, (bf16_t*)dx3, n8, HW, C);
    else
        hipLaunchKernelGGL(se_res_bwd_b_kernel<float>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<float>(dm), cp<float>(x3), mean3, rstd3,
                           g3, gate, rowscale, ds, s1, s2, inv_n, (float*)dx3, n8, HW, C);
    return ga_check_launch("ga_se_residual_bwd_b");
}

extern "C" int ga_subsample2_fwd(const void* x, void* y, int B, int H, int W, int C, int dtype, ga_stream_t stream) {
    GA_REQUIRE(x && y && B > 0 && H > 0 && W > 0 && (dtype == GA_BF16 || dtype == GA_F32), "ga_subsample2_fwd: bad args");
    if (int e = unsupported("ga_subsample2_fwd", (long)B * H * W, C)) return e;
    GA_REQUIRE(al16(x) && al16(y), "ga_subsample2_fwd: x and y must be 16-byte aligned");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long n8 = (long)B * Ho * Wo * (C / 8);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16)
        hipLaunchKernelGGL(subsample2_fwd_kernel<bf16_t>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<bf16_t>(x), (bf16_t*)y, H, W, C, Ho, Wo, n8);
    else
        hipLaunchKernelGGL(subsample2_fwd_kernel<float>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<float>(x), (float*)y, H, W, C, Ho, Wo, n8);
    return ga_check_launch("ga_subsample2_fwd");
}

extern "C" int ga_subsample2_bwd(const void* dy, void* dx, int B, int H, int W, int C, int accumulate, int dtype, ga_stream_t stream) {
    GA_REQUIRE(dy && dx && B > 0 && H > 0 && W > 0 && (dtype == GA_BF16 || dtype == GA_F32), "ga_subsample2_bwd: bad args");
    if (int e = unsupported("ga_subsample2_bwd", (long)B * H * W, C)) return e;
    GA_REQUIRE(al16(dy) && al16(dx), "ga_subsample2_bwd: dy and dx must be 16-byte aligned");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long n8 = (long)B * H * W * (C / 8);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16)
        hipLaunchKernelGGL(subsample2_bwd_kernel<bf16_t>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<bf16_t>(dy), (bf16_t*)dx, H, W, C, Ho,
                           Wo, n8, accumulate);
    else
        hipLaunchKernelGGL(subsample2_bwd_kernel<float>, dim3(blocks_for(n8)), dim3(kThreads), 0, s, cp<float>(dy), (float*)dx, H, W, C, Ho, Wo,
                           n8, accumulate);
    return ga_check_launch("ga_subsample2_bwd");
}
