// Depthwise 3x3 convolution (pad 1, stride 1 or 2, no bias), NHWC, for gfx950: the conv_dw layers of MobileNetV1
// (MAP/models/map_mobilenet.py:27-38).  HBM-bound VALU kernels, no MFMA (9 MAC per output element).
//
// One thread layout for all three kernels: a workgroup is (PL pixel lanes) x (CPB 8-channel chunks), CPB = min(C / 8, 64);
// gridDim.x walks the channel blocks, gridDim.y the pixel groups, and every thread keeps ONE 8-channel chunk for its whole
// life, so its 72 tap weights (w9 [C][9]: 72 contiguous floats) and its partial sums stay in registers.  Lanes of a wave
// read consecutive 16-byte channel chunks (C >= 512) or consecutive pixels of a narrow map (C = 32: 16 pixels x 64 B), so
// every load is a coalesced 16-byte access; the 3 x 3 neighbourhood re-reads hit L1 / L2.
//
//   fwd:         y = conv(x); optional BatchNorm batch sums of y (fp32, before rounding): per-thread partials, an ordered
//                LDS reduction over the pixel lanes, then ONE atomic per channel per workgroup (as ga_gemm's colsum epilogue)
//   bwd_data:    gather form -- each input pixel sums the <= 9 (stride 1) / <= 4 (stride 2) outputs that read it; no atomics
//   bwd_weight:  per-thread 72 partial sums -> ordered LDS reduction -> per-workgroup partials in the caller's workspace
//                [gy][C][9] -> one reduction launch that adds them, in pixel-group order, into dw9 (deterministic)
#include <algorithm>
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxCPB = 64;          // 8-channel chunks per workgroup
constexpr int kTargetWG = 2048;      // ~8 workgroups per CU (256 CUs)
constexpr long kWsFloats = 1L << 21; // bwd_weight partials: at most 8 MiB
constexpr int kWgradGroups = 512;    // bwd_weight: at most this many pixel groups (rows of partials the reduction reads)

struct Geo {
    int C8, CPB, PL, gx, gy;
};

Geo geometry(long npix, int C, bool wgrad) {
    Geo g;
    g.C8 = C / 8;
    g.CPB = std::min(g.C8, kMaxCPB);
    g.PL = kThreads / g.CPB;
    g.gx = (g.C8 + g.CPB - 1) / g.CPB;
    long gy = std::min<long>((npix + g.PL - 1) / g.PL, std::max(1, kTargetWG / g.gx));
    if (wgrad) gy = std::min<long>(std::min<long>(gy, kWgradGroups), std::max<long>(1, kWsFloats / (9L * C)));
    g.gy = (int)std::max<long>(1, gy);
    return g;
}

__device__ __forceinline__ void load_w72(const float* __restrict__ w9, int c, float w[9][8]) {
    // w9 [C][9]: the 8 channels c .. c+7 are 72 contiguous floats (16-byte aligned: c % 8 == 0 and 9 * 8 * 4 = 288)
    const float4* p = reinterpret_cast<const float4*>(w9 + (long)c * 9);
#pragma unroll
    for (int i = 0; i < 18; ++i) {
        const float4 v = p[i];
        const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = i * 4 + e;     // = j * 9 + k
            w[idx % 9][idx / 9] = f[e];
        }
    }
}

// ordered sum over the PL pixel lanes of v[8] (one chunk per thread): for every value r < CPB * 8 of the workgroup (chunk r / 8,
// channel r % 8; up to 512 values, so a thread may own two) calls out(r, sum); `red` is kThreads * 8 floats of LDS
template <typename Out>
__device__ __forceinline__ void lane_reduce(float* red, const float v[8], int t, int CPB, int PL, Out out) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[t * 8 + j] = v[j];
    __syncthreads();
    for (int r = t; r < CPB * 8; r += kThreads) {
        float s = 0.f;
        for (int p = 0; p < PL; ++p) s += red[p * CPB * 8 + r];
        out(r, s);
    }
    __syncthreads();
}

template <typename T, int S>
__global__ __launch_bounds__(kThreads) void dw3_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w9, T* __restrict__ y,
                                                           int B, int H, int W, int C, int Ho, int Wo, int CPB, int PL,
                                                           float* __restrict__ colsum, float* __restrict__ colsumsq) {
    __shared__ float red[kThreads * 8];
    const int t = threadIdx.x, cc = t % CPB, pl = t / CPB;
    const int chunk = blockIdx.x * CPB + cc;
    const bool active = pl < PL && chunk < C / 8;
    const int c = chunk * 8;
    float s[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.f;
    if (active) {
        float w[9][8];
        load_w72(w9, c, w);
        const long npix = (long)B * Ho * Wo;
        for (long p = (long)blockIdx.y * PL + pl; p < npix; p += (long)gridDim.y * PL) {
            const int ox = (int)(p % Wo);
            const long r = p / Wo;
            const int oy = (int)(r % Ho), b = (int)(r / Ho);
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = S * oy - 1 + ky;
                if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = S * ox - 1 + kx;
                    if ((unsigned)ix >= (unsigned)W) continue;
                    float xv[8];
                    load8(x + (((long)b * H + iy) * W + ix) * C + c, xv);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fmaf(w[ky * 3 + kx][j], xv[j], acc[j]);
                }
            }
            store8(y + p * C + c, acc);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                s[j] += acc[j];
                q[j] = fmaf(acc[j], acc[j], q[j]);
            }
        }
    }
    if (colsum == nullptr) return;       // (uniform over the grid: no thread is left waiting at a barrier)
    const int ch0 = blockIdx.x * CPB * 8;       // channel of value r: ch0 + r
    lane_reduce(red, s, t, CPB, PL, [&](int r, float v) { if (ch0 + r < C) atomicAdd(colsum + ch0 + r, v); });
    lane_reduce(red, q, t, CPB, PL, [&](int r, float v) { if (ch0 + r < C) atomicAdd(colsumsq + ch0 + r, v); });
}

// dx[b, iy, ix, c] = sum over taps (ky, kx) with S*oy - 1 + ky = iy, S*ox - 1 + kx = ix, 0 <= oy < Ho, 0 <= ox < Wo:
//                    w[c][ky*3+kx] * dy[b, oy, ox, c]
template <typename T, int S>
__global__ __launch_bounds__(kThreads) void dw3_bwd_data_kernel(const T* __restrict__ dy, const float* __restrict__ w9, T* __restrict__ dx,
                                                                int B, int H, int W, int C, int Ho, int Wo, int CPB, int PL) {
    const int t = threadIdx.x, cc = t % CPB, pl = t / CPB;
    const int chunk = blockIdx.x * CPB + cc;
    if (pl >= PL || chunk >= C / 8) return;
    const int c = chunk * 8;
    float w[9][8];
    load_w72(w9, c, w);
    const long npix = (long)B * H * W;
    for (long p = (long)blockIdx.y * PL + pl; p < npix; p += (long)gridDim.y * PL) {
        const int ix = (int)(p % W);
        const long r = p / W;
        const int iy = (int)(r % H), b = (int)(r / H);
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ty = iy + 1 - ky;
            if (ty < 0 || (S == 2 && (ty & 1))) continue;
            const int oy = ty / S;
            if (oy >= Ho) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int tx = ix + 1 - kx;
                if (tx < 0 || (S == 2 && (tx & 1))) continue;
                const int ox = tx / S;
                if (ox >= Wo) continue;
                float g[8];
                load8(dy + (((long)b * Ho + oy) * Wo + ox) * C + c, g);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = fmaf(w[ky * 3 + kx][j], g[j], acc[j]);
            }
        }
        store8(dx + p * C + c, acc);
    }
}

// part[blockIdx.y][c][k] = sum over this workgroup's output pixels of dy[b, oy, ox, c] * x[b, S*oy-1+ky, S*ox-1+kx, c]
template <typename T, int S>
__global__ __launch_bounds__(kThreads) void dw3_bwd_weight_kernel(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ part,
                                                                  int B, int H, int W, int C, int Ho, int Wo, int CPB, int PL) {
    __shared__ float red[kThreads * 8];
    const int t = threadIdx.x, cc = t % CPB, pl = t / CPB;
    const int chunk = blockIdx.x * CPB + cc;
    const bool active = pl < PL && chunk < C / 8;
    const int c = chunk * 8;
    float acc[9][8];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
    if (active) {
        const long npix = (long)B * Ho * Wo;
        for (long p = (long)blockIdx.y * PL + pl; p < npix; p += (long)gridDim.y * PL) {
            const int ox = (int)(p % Wo);
            const long r = p / Wo;
            const int oy = (int)(r % Ho), b = (int)(r / Ho);
            float g[8];
            load8(dy + p * C + c, g);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = S * oy - 1 + ky;
                if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = S * ox - 1 + kx;
                    if ((unsigned)ix >= (unsigned)W) continue;
                    float xv[8];
                    load8(x + (((long)b * H + iy) * W + ix) * C + c, xv);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[ky * 3 + kx][j] = fmaf(g[j], xv[j], acc[ky * 3 + kx][j]);
                }
            }
        }
    }
    float* out = part + (long)blockIdx.y * C * 9;
    const int ch0 = blockIdx.x * CPB * 8;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        lane_reduce(red, acc[k], t, CPB, PL, [&](int r, float v) { if (ch0 + r < C) out[(long)(ch0 + r) * 9 + k] = v; });
}

// dw9[e] += sum_g part[g][e], e < C * 9: a workgroup owns 64 consecutive e; its 4 waves take every 4th row g, each lane keeps 4
// independent partial sums (rows g, g + 4, ... in a fixed rotation), then a fixed-order combine -- deterministic, and 16 loads in
// flight per lane instead of one chain of G dependent loads
__global__ __launch_bounds__(kThreads) void dw3_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw9, int n, int G) {
    __shared__ float red[kThreads];
    const int t = threadIdx.x, lane = t % 64, q = t / 64;
    const int e = blockIdx.x * 64 + lane;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (e < n) {
        int g = q, i = 0;
        for (; g + 12 < G; g += 16)
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] += part[(long)(g + 4 * u) * n + e];
        for (; g < G; g += 4, ++i) a[i & 3] += part[(long)g * n + e];
    }
    red[t] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    if (q == 0 && e < n) dw9[e] += (red[lane] + red[64 + lane]) + (red[128 + lane] + red[192 + lane]);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_shape(const char* who, int B, int H, int W, int C, int stride) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || (stride != 1 && stride != 2) ||
        (long)B * H * W * C >= (1L << 40)) {
        ga_set_error("%s: unsupported shape (B %d, H %d, W %d, C %d, stride %d): C must be a multiple of 8, stride 1 or 2",
                     who, B, H, W, C, stride);
        return GA_ERR_UNSUPPORTED;
    }
    return GA_OK;
}

}  // namespace

extern "C" int ga_dwconv3_fwd(const void* x, const float* w9, void* y, int B, int H, int W, int C, int stride, float* colsum,
                              float* colsumsq, int dtype, ga_stream_t stream) {
    GA_REQUIRE(x && w9 && y && (colsum == nullptr) == (colsumsq == nullptr) && (dtype == GA_BF16 || dtype == GA_F32),
               "ga_dwconv3_fwd: bad args (colsum and colsumsq go together)");
    if (int e = check_shape("ga_dwconv3_fwd", B, H, W, C, stride)) return e;
    GA_REQUIRE(aligned16(x) && aligned16(y) && aligned16(w9), "ga_dwconv3_fwd: x, y and w9 must be 16-byte aligned");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const Geo g = geometry((long)B * Ho * Wo, C, false);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16) {
        using T = bf16_t;
        if (stride == 1)
            hipLaunchKernelGGL((dw3_fwd_kernel<T, 1>), dim3(g.gx, g.gy), dim3(kThreads), 0, s, (const T*)x, w9, (T*)y, B, H, W, C, Ho, Wo,
                               g.CPB, g.PL, colsum, colsumsq);
        else
            hipLaunchKernelGGL((dw3_fwd_kernel<T, 2>), dim3(g.gx, g.gy), dim3(kThreads), 0, s, (const T*)x, w9, (T*)y, B, H, W, C, Ho, Wo,
                               g.CPB, g.PL, colsum, colsumsq);
    } else {
        using T = float;
        if (stride == 1)
            hipLaunchKernelGGL((dw3_fwd_kernel<T, 1>), dim3(g.gx, g.gy), dim3(kThreads), 0, s, (const T*)x, w9, (T*)y, B, H, W, C, Ho, Wo,
                               g.CPB, g.PL, colsum, colsumsq);
        else
            hipLaunchKernelGGL((dw3_fwd_kernel<T, 2>), dim3(g.gx, g.gy), dim3(kThreads), 0, s, (const T*)x, w9, (T*)y, B, H, W, C, Ho, Wo,
                               g.CPB, g.PL, colsum, colsumsq);
    }
    return ga_check_launch("ga_dwconv3_fwd");
}

extern "C" int ga_dwconv3_bwd_data(const void* dy, const float* w9, void* dx, int B, int H, int W, int C, int stride, int dtype,
                                   ga_stream_t stream) {
    GA_REQUIRE(dy && w9 && dx && (dtype == GA_BF16 || dtype == GA_F32), "ga_dwconv3_bwd_data: bad args");
    if (int e = check_shape("ga_dwconv3_bwd_data", B, H, W, C, stride)) return e;
    GA_REQUIRE(aligned16(dy) && aligned16(dx) && aligned16(w9), "ga_dwconv3_bwd_data: dy, dx and w9 must be 16-byte aligned");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const Geo g = geometry((long)B * H * W, C, false);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16) {
        using T = bf16_t;
        if (stride == 1)
            hipLaunchKernelGGL((dw3_bwd_data_kernel<T, 1>), dim3(g.gx, g.gy), dim3(kThreads), 0, s, (const T*)dy, w9, (T*)dx, B, H, W, C, Ho,
                               Wo, g.CPB, g.PL);
        else
            hipLaunchKernelGGL((dw3_bwd_data_kernel<T, 2>), dim3(g.gx, g.gy), dim3(kThreads), 0, s, (const T*)dy, w9, (T*)dx, B, H, W, C, Ho,
                               Wo, g.CPB, g.PL);
    } else {
        using T = float;
        if (stride == 1)
            hipLaunchKernelGGL((dw3_bwd_data_kernel<T, 1>), dim3(g.gx, g.gy), dim3(kThreads), 0, s, (const T*)dy, w9, (T*)dx, B, H, W, C, Ho,
                               Wo, g.CPB, g.PL);
        else
            hipLaunchKernelGGL((dw3_bwd_data_kernel<T, 2>), dim3(g.gx, g.gy), dim3(kThreads), 0, s, (const T*)dy, w9, (T*)dx, B, H, W, C, Ho,
                               Wo, g.CPB, g.PL);
    }
    return ga_check_launch("ga_dwconv3_bwd_data");
}

extern "C" size_t ga_dwconv3_bwd_weight_workspace(int B, int H, int W, int C, int stride, int dtype) {
    (void)dtype;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || (stride != 1 && stride != 2)) return 0;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const Geo g = geometry((long)B * Ho * Wo, C, true);
    return (size_t)g.gy * C * 9 * sizeof(float);
}

extern "C" int ga_dwconv3_bwd_weight(const void* dy, const void* x, float* dw9, int B, int H, int W, int C, int stride, int dtype,
                                     void* workspace, size_t ws_bytes, ga_stream_t stream) {
    GA_REQUIRE(dy && x && dw9 && (dtype == GA_BF16 || dtype == GA_F32), "ga_dwconv3_bwd_weight: bad args");
    if (int e = check_shape("ga_dwconv3_bwd_weight", B, H, W, C, stride)) return e;
    GA_REQUIRE(aligned16(dy) && aligned16(x), "ga_dwconv3_bwd_weight: dy and x must be 16-byte aligned");
    const size_t need = ga_dwconv3_bwd_weight_workspace(B, H, W, C, stride, dtype);
    if (workspace == nullptr || ws_bytes < need) {
        ga_set_error("ga_dwconv3_bwd_weight: needs %zu B of caller-provided workspace (ga_dwconv3_bwd_weight_workspace), got %zu", need,
                     workspace ? ws_bytes : (size_t)0);
        return GA_ERR_BAD_ARG;
    }
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const Geo g = geometry((long)B * Ho * Wo, C, true);
    float* part = static_cast<float*>(workspace);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == GA_BF16) {
        using T = bf16_t;
        if (stride == 1)
            hipLaunchKernelGGL((dw3_bwd_weight_kernel<T, 1>), dim3(g.gx, g.gy), dim3(kThreads), 0, s, (const T*)dy, (const T*)x, part, B, H, W,
                               C, Ho, Wo, g.CPB, g.PL);
        else
            hipLaunchKernelGGL((dw3_bwd_weight_kernel<T, 2>), dim3(g.gx, g.gy), dim3(kThreads), 0, s, (const T*)dy, (const T*)x, part, B, H, W,
                               C, Ho, Wo, g.CPB, g.PL);
    } else {
        using T = float;
        if (stride == 1)
            hipLaunchKernelGGL((dw3_bwd_weight_kernel<T, 1>), dim3(g.gx, g.gy), dim3(kThreads), 0, s, (const T*)dy, (const T*)x, part, B, H, W,
                               C, Ho, Wo, g.CPB, g.PL);
        else
            hipLaunchKernelGGL((dw3_bwd_weight_kernel<T, 2>), dim3(g.gx, g.gy), dim3(kThreads), 0, s, (const T*)dy, (const T*)x, part, B, H, W,
                               C, Ho, Wo, g.CPB, g.PL);
    }
    if (int e = ga_check_launch("ga_dwconv3_bwd_weight")) return e;
    const int n = C * 9;
    hipLaunchKernelGGL(dw3_wgrad_reduce_kernel, dim3((n + 63) / 64), dim3(kThreads), 0, s, part, dw9, n, g.gy);
    return ga_check_launch("ga_dwconv3_bwd_weight.reduce");
}
