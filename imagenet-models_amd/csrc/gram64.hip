// float64 Gram vector of GA_ConvNeXt.get_gram's `training and B < 128` branch (ga_convnext.py:452-467).
//
// The reference divides x by H in the input dtype, casts to float64, and runs bmm, / (H W), the upper-triangular gather and
// F.normalize in float64; only the result goes back through .float().  The gradient comes back the same way: float64 down to the
// cast, rounded to the input dtype there, then / H in that dtype.  These kernels restate exactly that, with one rounding at each of
// the reference's casts.  B < 128 by definition: latency kernels on plain fp64 VALU FMAs, fixed summation order, no atomics.
#include "common.h"

namespace {

constexpr int GT = 32;   // tile edge of the Gram matrix / of dX (256 threads, 2 x 2 outputs each)
constexpr int GK = 32;   // reduction chunk staged in LDS

// x / H formed in the input dtype (one rounding to fp32 or bf16), then widened
template <typename T> __device__ __forceinline__ double xhat(const T* p, float Hf) {
    return (double)elt<T>::round(__fdiv_rn(elt<T>::ld(p), Hf));
}

// double -> fp32 rounded to odd: the RNE step to bf16 behind it then is the ONE rounding of the double value (fp32 keeps 16 more
// significand bits than bf16, so the sticky bit survives)
__device__ __forceinline__ float d2f_odd(double d) {
    float f = (float)d;
    if ((double)f != d) {
        unsigned u = __float_as_uint(f);
        if (fabs((double)f) > fabs(d)) --u;   // back to the neighbour towards zero
        f = __uint_as_float(u | 1u);
    }
    return f;
}
template <typename T> __device__ __forceinline__ T round_once(double d);
template <> __device__ __forceinline__ float round_once<float>(double d) { return (float)d; }
template <> __device__ __forceinline__ bf16_t round_once<bf16_t>(double d) { return f2bf(d2f_odd(d)); }
// the conversion torch applies where the reference casts a float64 gradient back to the input dtype (x.to(torch.float64) in
// backward): double -> bf16 goes through fp32 there, two RNE steps, and the backward follows it bit for bit
template <typename T> __device__ __forceinline__ T cast_back(double d);
template <> __device__ __forceinline__ float cast_back<float>(double d) { return (float)d; }
template <> __device__ __forceinline__ bf16_t cast_back<bf16_t>(double d) { return f2bf((float)d); }

// sum over the 1024 threads of a workgroup in a fixed order; every thread gets the total
__device__ __forceinline__ double block_sum_1024(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                   // red may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += red[w];
    return tot;
}

__device__ __forceinline__ long tri_index(int i, int j, int C) {   // packed row-major position of (i, j), i <= j
    return (long)i * C - (long)i * (i - 1) / 2 + (j - i);
}

// One workgroup per (sample, upper tile of G): G64[b][t(i, j)] = sum_p xh[p][i] xh[p][j] / HW for i <= j, p ascending.
template <typename T>
__global__ __launch_bounds__(256) void gram64_tile_kernel(const T* __restrict__ x, double* __restrict__ G64, int HW, int C,
                                                          int ntile, float Hf, long ntri) {
    __shared__ double As[GK][GT], Bs[GK][GT];
    const long b = blockIdx.x;
    int bi = 0, rem = blockIdx.y;
    while (rem >= ntile - bi) { rem -= ntile - bi; ++bi; }
    const int i0 = bi * GT, j0 = (bi + rem) * GT;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const T* xb = x + b * HW * C;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int p0 = 0; p0 < HW; p0 += GK) {
        for (int e = threadIdx.x; e < GK * GT; e += 256) {
            const int r = e >> 5, c = e & 31, p = p0 + r;
            As[r][c] = (p < HW && i0 + c < C) ? xhat(xb + (long)p * C + i0 + c, Hf) : 0.0;
            Bs[r][c] = (p < HW && j0 + c < C) ? xhat(xb + (long)p * C + j0 + c, Hf) : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < GK; ++kk) {
            const double a0 = As[kk][2 * ty], a1 = As[kk][2 * ty + 1], b0 = Bs[kk][2 * tx], b1 = Bs[kk][2 * tx + 1];
            acc[0][0] = fma(a0, b0, acc[0][0]);
            acc[0][1] = fma(a0, b1, acc[0][1]);
            acc[1][0] = fma(a1, b0, acc[1][0]);
            acc[1][1] = fma(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
    double* Gb = G64 + b * ntri;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int i = i0 + 2 * ty + u, j = j0 + 2 * tx + v;
            if (i < C && j < C && i <= j) Gb[tri_index(i, j, C)] = acc[u][v] / (double)HW;
        }
}

// One workgroup per sample: norm over the packed entries, 1 / max(norm, 1e-12) kept as a double, the normalised vector rounded
// once into [groups][Kp] (pad columns zero).
template <typename T>
__global__ __launch_bounds__(1024) void gram64_pack_kernel(const double* __restrict__ G64, T* __restrict__ out,
                                                           double* __restrict__ inv_norm, int ntri, int groups, int Kg, int Kp) {
    __shared__ double red[16];
    const long b = blockIdx.x;
    const double* Gb = G64 + b * ntri;
    double ss = 0.0;
    for (int t = threadIdx.x; t < ntri; t += 1024) ss = fma(Gb[t], Gb[t], ss);
    const double denom = fmax(sqrt(block_sum_1024(ss, red)), 1e-12);
    if (threadIdx.x == 0) inv_norm[b] = 1.0 / denom;
    T* ob = out + b * groups * Kp;
    for (int e = threadIdx.x; e < groups * Kp; e += 1024) {
        const int g = e / Kp, k = e - g * Kp;
        ob[e] = k < Kg ? round_once<T>(Gb[g * Kg + k] / denom) : (T)0;
    }
}

// Backward of normalise + gather, one workgroup per sample: S64[b][i][j] (symmetric, diagonal doubled) = d(raw Gram entry)
//   d_raw = (dvec - vhat <vhat, dvec>) / norm      with vhat = G64 / norm in double (never the rounded vec)
template <typename T>
__global__ __launch_bounds__(1024) void gram64_bwd_s_kernel(const T* __restrict__ dvec, const double* __restrict__ G64,
                                                            const double* __restrict__ inv_norm, double* __restrict__ S64, int C,
                                                            int ntri, int groups, int Kg, int Kp) {
    __shared__ double red[16];
    const long b = blockIdx.x;
    const double* Gb = G64 + b * ntri;
    const T* db = dvec + b * groups * Kp;
    const double inv = inv_norm[b];
    double dot = 0.0;
    for (int t = threadIdx.x; t < ntri; t += 1024) {
        const int g = t / Kg, k = t - g * Kg;
        dot = fma(Gb[t] * inv, (double)elt<T>::ld(db + g * Kp + k), dot);
    }
    dot = block_sum_1024(dot, red);
    if (inv >= 1e12) dot = 0.0;          // norm clamped at 1e-12: F.normalize then is a plain division by the constant
    double* Sb = S64 + b * C * C;
    for (int e = threadIdx.x; e < C * C; e += 1024) {
        const int i = e / C, j = e - i * C;
        const int t = (int)tri_index(min(i, j), max(i, j), C);
        const int g = t / Kg, k = t - g * Kg;
        const double draw = inv * ((double)elt<T>::ld(db + g * Kp + k) - Gb[t] * inv * dot);
        Sb[e] = i == j ? 2.0 * draw : draw;
    }
}

// dXh[b][p][i] = sum_j xh[p][j] S64[j][i] / HW in double (j ascending), cast to the input dtype as the reference's backward of
// .to(torch.float64) does, then / H in that dtype.  One workgroup per (32 positions, 32 channels, sample).
template <typename T>
__global__ __launch_bounds__(256) void gram64_dx_kernel(const T* __restrict__ x, const double* __restrict__ S64, T* __restrict__ dx,
                                                        int HW, int C, float Hf) {
    __shared__ double As[GK][GT + 1], Bs[GK][GT];
    const long b = blockIdx.z;
    const int p0 = blockIdx.x * GT, i0 = blockIdx.y * GT;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const T* xb = x + b * HW * C;
    const double* Sb = S64 + b * C * C;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int j0 = 0; j0 < C; j0 += GK) {
        for (int e = threadIdx.x; e < GK * GT; e += 256) {
            const int r = e >> 5, c = e & 31;
            As[c][r] = (p0 + r < HW && j0 + c < C) ? xhat(xb + (long)(p0 + r) * C + j0 + c, Hf) : 0.0;
            Bs[r][c] = (j0 + r < C && i0 + c < C) ? Sb[(long)(j0 + r) * C + i0 + c] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < GK; ++kk) {
            const double a0 = As[kk][2 * ty], a1 = As[kk][2 * ty + 1], b0 = Bs[kk][2 * tx], b1 = Bs[kk][2 * tx + 1];
            acc[0][0] = fma(a0, b0, acc[0][0]);
            acc[0][1] = fma(a0, b1, acc[0][1]);
            acc[1][0] = fma(a1, b0, acc[1][0]);
            acc[1][1] = fma(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
    T* db = dx + b * HW * C;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int p = p0 + 2 * ty + u, i = i0 + 2 * tx + v;
            if (p < HW && i < C) {
                const T g = cast_back<T>(acc[u][v] / (double)HW);
                elt<T>::st(db + (long)p * C + i, __fdiv_rn(elt<T>::ld(&g), Hf));
            }
        }
}

bool gram64_args_ok(int B, int HW, int C, int H, int groups, int Kp, int dtype) {
    if (B < 1 || HW < 1 || C < 8 || C % 8 || C > 4096 || H < 1 || groups < 1 || (dtype != GA_F32 && dtype != GA_BF16)) return false;
    const int ntri = C * (C + 1) / 2;
    return ntri % groups == 0 && Kp >= ntri / groups;
}

}  // namespace

extern "C" size_t ga_gram_f64_fwd_workspace(int B, int C) {
    return B < 1 || C < 1 ? 0 : (size_t)B * ((size_t)C * (C + 1) / 2) * sizeof(double);
}

extern "C" size_t ga_gram_f64_bwd_workspace(int B, int C) {
    return B < 1 || C < 1 ? 0 : (size_t)B * C * C * sizeof(double);
}

extern "C" int ga_gram_f64_fwd(const void* x, void* vec, double* inv_norm, double* G64, size_t g64_bytes, int B, int HW, int C,
                               int H, int groups, int Kp, int dtype, ga_stream_t stream) {
    GA_REQUIRE(gram64_args_ok(B, HW, C, H, groups, Kp, dtype),
               "ga_gram_f64_fwd: bad args (B=%d HW=%d C=%d H=%d groups=%d Kp=%d dtype=%d)", B, HW, C, H, groups, Kp, dtype);
    GA_REQUIRE(x && vec && inv_norm && G64 && ((uintptr_t)G64 & 7) == 0 && ((uintptr_t)inv_norm & 7) == 0,
               "ga_gram_f64_fwd: null or misaligned pointer");
    GA_REQUIRE(g64_bytes >= ga_gram_f64_fwd_workspace(B, C), "ga_gram_f64_fwd: G64 holds %zu bytes, needs %zu", g64_bytes,
               ga_gram_f64_fwd_workspace(B, C));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int ntri = C * (C + 1) / 2, ntile = cdiv(C, GT);
    if (dtype == GA_BF16) {
        hipLaunchKernelGGL(gram64_tile_kernel<bf16_t>, dim3(B, ntile * (ntile + 1) / 2), dim3(256), 0, s, (const bf16_t*)x, G64, HW, C,
                           ntile, (float)H, (long)ntri);
        hipLaunchKernelGGL(gram64_pack_kernel<bf16_t>, dim3(B), dim3(1024), 0, s, G64, (bf16_t*)vec, inv_norm, ntri, groups,
                           ntri / groups, Kp);
    } else {
        hipLaunchKernelGGL(gram64_tile_kernel<float>, dim3(B, ntile * (ntile + 1) / 2), dim3(256), 0, s, (const float*)x, G64, HW, C,
                           ntile, (float)H, (long)ntri);
        hipLaunchKernelGGL(gram64_pack_kernel<float>, dim3(B), dim3(1024), 0, s, G64, (float*)vec, inv_norm, ntri, groups,
                           ntri / groups, Kp);
    }
    return ga_check_launch("ga_gram_f64_fwd");
}

extern "C" int ga_gram_f64_bwd(const void* dvec, const void* x, const double* G64, const double* inv_norm, void* dx, void* workspace,
                               size_t ws_bytes, int B, int HW, int C, int H, int groups, int Kp, int dtype, ga_stream_t stream) {
    GA_REQUIRE(gram64_args_ok(B, HW, C, H, groups, Kp, dtype),
               "ga_gram_f64_bwd: bad args (B=%d HW=%d C=%d H=%d groups=%d Kp=%d dtype=%d)", B, HW, C, H, groups, Kp, dtype);
    GA_REQUIRE(dvec && x && G64 && inv_norm && dx && workspace && ((uintptr_t)G64 & 7) == 0 && ((uintptr_t)inv_norm & 7) == 0 &&
                   ((uintptr_t)workspace & 7) == 0,
               "ga_gram_f64_bwd: null or misaligned pointer");
    GA_REQUIRE(ws_bytes >= ga_gram_f64_bwd_workspace(B, C), "ga_gram_f64_bwd: workspace holds %zu bytes, needs %zu", ws_bytes,
               ga_gram_f64_bwd_workspace(B, C));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int ntri = C * (C + 1) / 2;
    double* S64 = reinterpret_cast<double*>(workspace);
    const dim3 grid(cdiv(HW, GT), cdiv(C, GT), B);
    if (dtype == GA_BF16) {
        hipLaunchKernelGGL(gram64_bwd_s_kernel<bf16_t>, dim3(B), dim3(1024), 0, s, (const bf16_t*)dvec, G64, inv_norm, S64, C, ntri,
                           groups, ntri / groups, Kp);
        hipLaunchKernelGGL(gram64_dx_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, S64, (bf16_t*)dx, HW, C, (float)H);
    } else {
        hipLaunchKernelGGL(gram64_bwd_s_kernel<float>, dim3(B), dim3(1024), 0, s, (const float*)dvec, G64, inv_norm, S64, C, ntri,
                           groups, ntri / groups, Kp);
        hipLaunchKernelGGL(gram64_dx_kernel<float>, grid, dim3(256), 0, s, (const float*)x, S64, (float*)dx, HW, C, (float)H);
    }
    return ga_check_launch("ga_gram_f64_bwd");
}
