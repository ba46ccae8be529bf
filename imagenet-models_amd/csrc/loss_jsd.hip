// Jensen-Shannon consistency loss over augmentation splits (timm JsdCrossEntropy, GA/train.py:613-615) fused with the head
// decorrelation and the MAP self-distillation terms of ga_loss_kernel: forward + gradient in one launch (gfx950).
#include "common.h"

namespace {

constexpr int JSD_MAX_SPLITS = 8;

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
    return s;
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = -3.0e38f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s = fmaxf(s, red[i]);
    return s;
}
// log-sum-exp of one row of NC logits: max, sum of __expf(x - max), max + __logf(sum)
__device__ __forceinline__ float block_lse(const float* __restrict__ x, int NC, float* red) {
    float m = -3.0e38f;
    for (int c = threadIdx.x; c < NC; c += 256) m = fmaxf(m, x[c]);
    m = block_max(m, red);
    float s = 0.f;
    for (int c = threadIdx.x; c < NC; c += 256) s += __expf(x[c] - m);
    s = block_sum(s, red);
    return m + __logf(s);
}

// One workgroup per BASE sample i: it owns the S rows i + s Bs (split-major batch, Bs = B / S) of all K heads.
//   loss = sum_k [ CE_smooth(out_k[split 0], y) (mean over Bs)
//                  + alpha / S * sum_s sum_c p_s (log p_s - log m) / Bs,    m = clamp(mean_s p_s, 1e-7, 1)
//                  + lam * KL_mean(log_softmax(out_k) || log_softmax(mean_j out_j))  (all B rows, mean target detached)
//                  + (avg) sum_bc p_k (log p_k - log softmax(avg_k)) / (B NC)        (all B rows) ]
// log p is always x - lse; log m is the one logarithm of a probability.  The clamp passes no gradient outside [1e-7, 1]:
//   g_sc = A [ (log p_sc - log m_c) + (clamped ? 1 : 0) ],  A = alpha / B;   d/dx_sc = p_sc (g_sc - sum_c' p_sc' g_sc')
// LDS: the S log r rows (log_softmax of the mean over heads) + 8 floats of reduction scratch.
template <typename T>
__global__ __launch_bounds__(256) void ga_loss_jsd_kernel(const float* __restrict__ org, const float* __restrict__ avg,
                                                          const int64_t* __restrict__ target, float* __restrict__ loss,
                                                          T* __restrict__ dorg, T* __restrict__ davg, int K, int B, int NC, int S,
                                                          float lam, float smooth, float alpha, float gscale) {
    extern __shared__ float sm[];  // logr[S][NC]; red[8]
    float* red = sm + (long)S * NC;
    const int Bs = B / S;
    const long i = blockIdx.x;
    const int y = (int)target[i];
    const float invBs = 1.f / (float)Bs, invBN = 1.f / ((float)B * (float)NC), A = alpha / (float)B;
    const float off = smooth / (float)NC, on = 1.f - smooth + off;
    // log r = log_softmax(mean_k out_k) of each of the S rows
    for (int s = 0; s < S; ++s) {
        float* r = sm + (long)s * NC;
        const long b = i + (long)s * Bs;
        for (int c = threadIdx.x; c < NC; c += 256) {
            float m = 0.f;
            for (int k = 0; k < K; ++k) m += org[((long)k * B + b) * NC + c];
            r[c] = m / (float)K;
        }
        __syncthreads();
        const float lse_r = block_lse(r, NC, red);
        for (int c = threadIdx.x; c < NC; c += 256) r[c] = r[c] - lse_r;
    }
    __syncthreads();
    float total = 0.f;  // this thread's share of the loss
    for (int k = 0; k < K; ++k) {
        const float* o = org + ((long)k * B + i) * NC;      // row of split s: o + s Bs NC
        const long sstr = (long)Bs * NC;
        float lse[JSD_MAX_SPLITS], dot[JSD_MAX_SPLITS];
#pragma unroll
        for (int s = 0; s < JSD_MAX_SPLITS; ++s) {
            lse[s] = 0.f;
            dot[s] = 0.f;
            if (s < S) lse[s] = block_lse(o + s * sstr, NC, red);
        }
        // pass 1: the JSD value and the softmax-Jacobian dot products sum_c p_sc g_sc
        for (int c = threadIdx.x; c < NC; c += 256) {
            float lp[JSD_MAX_SPLITS], p[JSD_MAX_SPLITS], q = 0.f;
#pragma unroll
            for (int s = 0; s < JSD_MAX_SPLITS; ++s)
                if (s < S) {
                    lp[s] = o[s * sstr + c] - lse[s];
                    p[s] = __expf(lp[s]);
                    q += p[s];
                }
            q /= (float)S;
            const float logm = __logf(fminf(fmaxf(q, 1e-7f), 1.f));
            const float extra = (q >= 1e-7f && q <= 1.f) ? 0.f : 1.f;
#pragma unroll
            for (int s = 0; s < JSD_MAX_SPLITS; ++s)
                if (s < S) {
                    const float d = lp[s] - logm;
                    total += A * (p[s] * d);
                    dot[s] += p[s] * (A * (d + extra));
                }
        }
#pragma unroll
        for (int s = 0; s < JSD_MAX_SPLITS; ++s)
            if (s < S) dot[s] = block_sum(dot[s], red);
        // pass 2: every gradient element, written once
        for (int c = threadIdx.x; c < NC; c += 256) {
            float lp[JSD_MAX_SPLITS], p[JSD_MAX_SPLITS], q = 0.f;
#pragma unroll
            for (int s = 0; s < JSD_MAX_SPLITS; ++s)
                if (s < S) {
                    lp[s] = o[s * sstr + c] - lse[s];
                    p[s] = __expf(lp[s]);
                    q += p[s];
                }
            q /= (float)S;
            const float logm = __logf(fminf(fmaxf(q, 1e-7f), 1.f));
            const float extra = (q >= 1e-7f && q <= 1.f) ? 0.f : 1.f;
#pragma unroll
            for (int s = 0; s < JSD_MAX_SPLITS; ++s)
                if (s < S) {
                    const float logr = sm[(long)s * NC + c], rr = __expf(logr);
                    total += lam * rr * (logr - lp[s]) * invBN;
                    float g = lam * invBN * (p[s] - rr);
                    g += p[s] * (A * ((lp[s] - logm) + extra) - dot[s]);
                    if (s == 0) {
                        const float t = (c == y) ? on : off;
                        total += -t * lp[0] * invBs;
                        g += (p[0] - t) * invBs;
                    }
                    if (dorg) elt<T>::st(dorg + ((long)k * B + i) * NC + s * sstr + c, g * gscale);
                }
        }
        if (avg) {   // MAP self-distillation term, as in ga_loss_kernel, over every row
#pragma unroll
            for (int s = 0; s < JSD_MAX_SPLITS; ++s)
                if (s < S) {
                    const float* a = avg + ((long)k * B + i) * NC + s * sstr;
                    const float lse_a = block_lse(a, NC, red);
                    for (int c = threadIdx.x; c < NC; c += 256) {
                        const float logp = o[s * sstr + c] - lse[s], p = __expf(logp), loga = a[c] - lse_a;
                        total += p * (logp - loga) * invBN;
                        if (davg) elt<T>::st(davg + ((long)k * B + i) * NC + s * sstr + c, (__expf(loga) - p) * invBN * gscale);
                    }
                }
        }
    }
    total = block_sum(total, red);
    if (threadIdx.x == 0) atomicAdd(loss, total);
}

}  // namespace

extern "C" int ga_loss_jsd_fwd_bwd(const float* org, const float* avg, const int64_t* target, float* loss, void* dorg, void* davg,
                                   int K, int B, int NC, int num_splits, float lam, float smoothing, float alpha, float grad_scale,
                                   int dtype, ga_stream_t stream) {
    GA_REQUIRE(org && target && loss, "ga_loss_jsd_fwd_bwd: org, target and loss must be given");
    GA_REQUIRE(!(davg && !avg), "ga_loss_jsd_fwd_bwd: davg given without avg");
    GA_REQUIRE(K >= 1 && B >= 1 && NC >= 1, "ga_loss_jsd_fwd_bwd: bad shape K=%d B=%d NC=%d", K, B, NC);
    GA_REQUIRE(num_splits >= 2 && num_splits <= JSD_MAX_SPLITS, "ga_loss_jsd_fwd_bwd: num_splits=%d, supported 2..%d", num_splits,
               JSD_MAX_SPLITS);
    GA_REQUIRE(B % num_splits == 0, "ga_loss_jsd_fwd_bwd: batch %d is not a multiple of num_splits=%d", B, num_splits);
    const size_t lds = ((size_t)num_splits * NC + 8) * sizeof(float);
    GA_REQUIRE(lds <= 160 * 1024, "ga_loss_jsd_fwd_bwd: num_splits=%d x num_classes=%d rows need %zu B of LDS, above 160 KiB",
               num_splits, NC, lds);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (lds > 65536) {
        static const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(ga_loss_jsd_kernel<bf16_t>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
                               hipFuncSetAttribute(reinterpret_cast<const void*>(ga_loss_jsd_kernel<float>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
        GA_REQUIRE(ok, "ga_loss_jsd_fwd_bwd: cannot reserve %zu B of LDS", lds);
    }
    if (dtype == GA_BF16)
        hipLaunchKernelGGL(ga_loss_jsd_kernel<bf16_t>, dim3(B / num_splits), dim3(256), lds, s, org, avg, target, loss, (bf16_t*)dorg,
                           (bf16_t*)davg, K, B, NC, num_splits, lam, smoothing, alpha, grad_scale);
    else
        hipLaunchKernelGGL(ga_loss_jsd_kernel<float>, dim3(B / num_splits), dim3(256), lds, s, org, avg, target, loss, (float*)dorg,
                           (float*)davg, K, B, NC, num_splits, lam, smoothing, alpha, grad_scale);
    return ga_check_launch("ga_loss_jsd_fwd_bwd");
}
