// Device-side input augmentation of the training step: timm RandomErasing as PrefetchLoader applies it -- on the GPU, on the
// normalised batch, behind `.float().sub_(mean).div_(std)` and ahead of mixup (MAP/train.py:214-220,643-646: --reprob /
// --remode / --recount).  ga_input_erase is ga_u8_normalize (or a plain copy of an fp32 batch) with the erase boxes filled in
// the same pass: zeros ('const'), one N(0,1) colour per box and channel ('rand'), or N(0,1) per element ('pixel').
//
// The normals come from a counter-based generator, so the value at an element is a pure function of (seed, offset, index):
//
//   Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85)
//     key      k0 = seed[31:0]            k1 = seed[63:32]
//     counter  c0 = q[31:0]   c1 = q[63:32]   c2 = offset[31:0]   c3 = offset[62:32] | stream << 31
//   'pixel' (stream 0):  q = i >> 2 for the flat element index i = ((b*CH + c)*H + y)*W + x  -- one call per aligned group of four
//                        consecutive elements; element i takes normal n[i & 3]
//   'rand'  (stream 1):  q = (b*max_count + j)*CH + c for box j of sample b, channel c; the colour is n[0]
//   outputs r0..r3 -> uniforms u_k = ((r_k >> 9) + 0.5) * 2^-23  in (0, 1): 23 bits, exact in fp32, never 0 (no log(0)) or 1
//   Box-Muller:  n0 = R(u0) cos(2 pi u1)   n1 = R(u0) sin(2 pi u1)   n2 = R(u2) cos(2 pi u3)   n3 = R(u2) sin(2 pi u3)
//                R(u) = sqrt(-2 ln u)   (|n| <= sqrt(48 ln 2) = 5.77)
// evaluated with the accurate logf / sqrtf and sincospif(2 u) (no fast intrinsics; 2 u is exact, so no rounding of 2 pi u).
#include "common.h"

#include <algorithm>

namespace {
struct EraseCh { float mean[4], std[4]; };

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned r[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        // one 32 x 32 -> 64 multiply each (v_mad_u64_u32) instead of a mul_hi / mul_lo pair
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        c0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
        c1 = (unsigned)p1;
        c2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c3 = (unsigned)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ float unit23(unsigned r) { return ((float)(r >> 9) + 0.5f) * (1.0f / 8388608.0f); }

// the four normals of counter (q, offset, stream) under key seed
__device__ __forceinline__ void philox_normal4(unsigned long long q, unsigned long long offset, unsigned stream, unsigned long long seed,
                                               float n[4]) {
    unsigned r[4];
    philox4x32_10((unsigned)q, (unsigned)(q >> 32), (unsigned)offset, ((unsigned)(offset >> 32) & 0x7fffffffu) | (stream << 31),
                  (unsigned)seed, (unsigned)(seed >> 32), r);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float rad = sqrtf(-2.0f * logf(unit23(r[2 * k])));
        float s, c;
        sincospif(2.0f * unit23(r[2 * k + 1]), &s, &c);
        n[2 * k] = rad * c;
        n[2 * k + 1] = rad * s;
    }
}

// the covering box of each of the four elements behind (y, x) of a plane: the LAST box that holds it (timm erases in order), -1: none.
// MAXC = max_count for 1..4 (the table in SGPRs, loaded once), 0: any count, a loop of scalar loads.  A span inside one row --
// every span when W % 4 == 0 -- is first tested as a whole, which rejects nearly every (span, box) pair in four compares.
__device__ __forceinline__ void box_hits(const int4 q, int j, bool one_row, int y, int x, int W, int hit[4]) {   // q: top, left, h, w
    if (one_row) {
        if (y >= q.x && y < q.x + q.z && x + 3 >= q.y && x < q.y + q.w) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e >= q.y && x + e < q.y + q.w) hit[e] = j;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            while (x >= W) { x -= W; ++y; }
            if (y >= q.x && y < q.x + q.z && x >= q.y && x < q.y + q.w) hit[e] = j;
            ++x;
        }
    }
}

template <int MAXC>
__device__ __forceinline__ bool span_hits(const int4* __restrict__ bx, int max_count, int y, int x, int W, int hit[4]) {
    hit[0] = hit[1] = hit[2] = hit[3] = -1;
    const bool one_row = x + 3 < W;
    if constexpr (MAXC > 0) {
#pragma unroll
        for (int j = 0; j < MAXC; ++j) box_hits(bx[j], j, one_row, y, x, W, hit);
    } else {
        for (int j = 0; j < max_count; ++j) box_hits(bx[j], j, one_row, y, x, W, hit);
    }
    return (hit[0] & hit[1] & hit[2] & hit[3]) >= 0;       // any element covered
}

// grid (x, B): the workgroups of row b stride over the CH*HW/4 four-element groups of sample b, so the sample's box table is
// wave-uniform (scalar loads) and a sample without boxes takes the plain normalise / copy loop.
// 4 elements per thread (HW % 4 == 0): one 4-byte (uint8) or 16-byte (fp32) load, one 16-byte store
template <bool U8, int MAXC>
__global__ __launch_bounds__(256) void input_erase_kernel(const void* __restrict__ xin, float* __restrict__ out, int CH, int H, int W,
                                                          EraseCh nc, const int4* __restrict__ boxes, int max_count, int mode,
                                                          unsigned long long seed, unsigned long long offset) {
    const int b = blockIdx.y;
    const int HW = H * W, per = CH * HW;                    // < 2^30 (checked by the launcher)
    const int4* __restrict__ bx = boxes + (long)b * max_count;
    bool any = false;
    for (int j = 0; j < max_count; ++j) any |= bx[j].z > 0 && bx[j].w > 0;
    for (int p = (blockIdx.x * 256 + threadIdx.x) * 4; p < per; p += gridDim.x * 1024) {
        const long i = (long)b * per + p;                  // p: offset inside the sample, i: flat element index
        const int c = p / HW;
        float v[4];
        if (U8) {
            const unsigned u = *reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(xin) + i);
            const float m = nc.mean[c], s = nc.std[c];
            v[0] = ((float)(u & 255u) - m) / s;
            v[1] = ((float)((u >> 8) & 255u) - m) / s;
            v[2] = ((float)((u >> 16) & 255u) - m) / s;
            v[3] = ((float)(u >> 24) - m) / s;
        } else {
            load4(reinterpret_cast<const float*>(xin) + i, v);
        }
        if (any) {
            const int r = p - c * HW, y = r / W;
            int hit[4];
            if (span_hits<MAXC>(bx, max_count, y, r - y * W, W, hit)) {
                float n[4] = {0.f, 0.f, 0.f, 0.f};
                if (mode == 2) philox_normal4((unsigned long long)i >> 2, offset, 0u, seed, n);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (hit[e] < 0) continue;
                    if (mode == 1) {
                        float col[4];
                        philox_normal4((unsigned long long)(((long)b * max_count + hit[e]) * CH + c), offset, 1u, seed, col);
                        v[e] = col[0];
                    } else {
                        v[e] = n[e];
                    }
                }
            }
        }
        store4(out + i, v);
    }
}

template <bool U8>
void launch_input_erase(dim3 grid, hipStream_t s, const void* x, float* out, int CH, int H, int W, const EraseCh& nc, const int4* bx,
                        int max_count, int mode, unsigned long long seed, unsigned long long offset) {
#define GA_ERASE_LAUNCH(MAXC) \
    hipLaunchKernelGGL((input_erase_kernel<U8, MAXC>), grid, dim3(256), 0, s, x, out, CH, H, W, nc, bx, max_count, mode, seed, offset)
    switch (max_count) {
        case 1: GA_ERASE_LAUNCH(1); break;
        case 2: GA_ERASE_LAUNCH(2); break;
        case 3: GA_ERASE_LAUNCH(3); break;
        case 4: GA_ERASE_LAUNCH(4); break;
        default: GA_ERASE_LAUNCH(0); break;
    }
#undef GA_ERASE_LAUNCH
}

// ------------------------------------------------------------------------------------------------
// ga_input_collate: timm's collate-time order in one pass -- FastCollateMixup on the uint8 batch (mixup rounded back to uint8
// with round-half-to-even, cutmix a box copy), PrefetchLoader's normalisation, RandomErasing last on the mixed image.  Each
// sample carries its own mix row, so timm's modes 'batch', 'elem' and 'pair' are one kernel; the partner of sample b is B-1-b and
// everything reads the ORIGINAL batch (out of place).  The fp32 instantiation is timm's Mixup on a normalised batch: the same
// blend without the rounding to integers and without the normalisation.
//   mix row (32 bytes): kind (0 none, 1 mixup, 2 cutmix), yl, yh, xl, xh, bits(l), bits(m), 0   -- l / m: fp32 lam and complement
//   mixup : u8(rint(fl(fl(a*l) + fl(b*m))))   three separately rounded fp32 operations: never contracted into an FMA
//   cutmix: the partner's value inside [yl, yh) x [xl, xh), the sample's own outside
// ------------------------------------------------------------------------------------------------
struct MixRow { int kind, yl, yh, xl, xh; float l, m; };

// fl(fl(a*l) + fl(b*m)).  hipcc contracts a*l + b*m into an FMA by default, and __fmul_rn / __fadd_rn are plain * and + in its
// headers (they inline and contract as well): the pragma is what keeps the three roundings apart, as in mixup_batch_kernel
__device__ __forceinline__ float blend_rn(float a, float b, float l, float m) {
#pragma clang fp contract(off)
    const float p = a * l, q = b * m;
    return p + q;
}

__device__ __forceinline__ void unpack_u8(unsigned u, float v[4]) {
    v[0] = (float)(u & 255u); v[1] = (float)((u >> 8) & 255u); v[2] = (float)((u >> 16) & 255u); v[3] = (float)(u >> 24);
}

// the loop of one sample for a compile-time KIND: the branch on the kind is taken once per sample (collate_kernel), not here
template <bool U8, int MAXC, int KIND>
__device__ __forceinline__ void collate_sample(const void* __restrict__ xin, float* __restrict__ out, int b, int pb, int CH, int H, int W,
                                               const EraseCh& nc, const MixRow mr, const int4* __restrict__ bx, int max_count, bool any,
                                               int mode, unsigned long long seed, unsigned long long offset) {
    const int HW = H * W, per = CH * HW;                    // < 2^30 (checked by the launcher)
    const int4 cut = make_int4(mr.yl, mr.xl, mr.yh - mr.yl, mr.xh - mr.xl);      // top, left, h, w: an empty box hits nothing
    for (int p = (blockIdx.x * 256 + threadIdx.x) * 4; p < per; p += gridDim.x * 1024) {
        const long i = (long)b * per + p, j = (long)pb * per + p;     // own / partner element: the same offset inside the sample
        const int c = p / HW;
        const int r = p - c * HW, y = r / W, x = r - y * W;
        float v[4];
        if (U8) unpack_u8(*reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(xin) + i), v);
        else load4(reinterpret_cast<const float*>(xin) + i, v);
        if (KIND == 1) {
            float w[4];
            if (U8) unpack_u8(*reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(xin) + j), w);
            else load4(reinterpret_cast<const float*>(xin) + j, w);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = blend_rn(v[e], w[e], mr.l, mr.m);
                v[e] = U8 ? rintf(t) : t;                   // rintf: round half to even (np.rint); an integer 0..255, exact in fp32
            }
        } else if (KIND == 2) {
            int in[4] = {-1, -1, -1, -1};
            box_hits(cut, 0, x + 3 < W, y, x, W, in);
            if ((in[0] & in[1] & in[2] & in[3]) >= 0) {     // the partner is read only by spans that touch the box
                float w[4];
                if (U8) unpack_u8(*reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(xin) + j), w);
                else load4(reinterpret_cast<const float*>(xin) + j, w);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (in[e] >= 0) v[e] = w[e];
            }
        }
        if (U8) {
            const float m = nc.mean[c], s = nc.std[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (v[e] - m) / s;
        }
        if (any) {
            int hit[4];
            if (span_hits<MAXC>(bx, max_count, y, x, W, hit)) {
                float n[4] = {0.f, 0.f, 0.f, 0.f};
                if (mode == 2) philox_normal4((unsigned long long)i >> 2, offset, 0u, seed, n);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (hit[e] < 0) continue;
                    if (mode == 1) {
                        float col[4];
                        philox_normal4((unsigned long long)(((long)b * max_count + hit[e]) * CH + c), offset, 1u, seed, col);
                        v[e] = col[0];
                    } else {
                        v[e] = n[e];
                    }
                }
            }
        }
        store4(out + i, v);
    }
}

// grid (x, B) as input_erase_kernel: the mix row and the erase boxes of sample b are wave-uniform (scalar loads); a 'none' sample
// without boxes runs the plain normalise / copy loop
template <bool U8, int MAXC>
__global__ __launch_bounds__(256) void input_collate_kernel(const void* __restrict__ xin, float* __restrict__ out, int CH, int H, int W,
                                                            EraseCh nc, const int4* __restrict__ mix, const int4* __restrict__ boxes,
                                                            int max_count, int mode, unsigned long long seed,
                                                            unsigned long long offset) {
    const int b = blockIdx.y, pb = gridDim.y - 1 - b;
    const int4 m0 = mix[2 * b], m1 = mix[2 * b + 1];
    const MixRow mr = {m0.x, m0.y, m0.z, m0.w, m1.x, __int_as_float(m1.y), __int_as_float(m1.z)};
    const int4* __restrict__ bx = boxes + (long)b * max_count;
    bool any = false;
    for (int j = 0; j < max_count; ++j) any |= bx[j].z > 0 && bx[j].w > 0;
    if (mr.kind == 1) collate_sample<U8, MAXC, 1>(xin, out, b, pb, CH, H, W, nc, mr, bx, max_count, any, mode, seed, offset);
    else if (mr.kind == 2) collate_sample<U8, MAXC, 2>(xin, out, b, pb, CH, H, W, nc, mr, bx, max_count, any, mode, seed, offset);
    else collate_sample<U8, MAXC, 0>(xin, out, b, pb, CH, H, W, nc, mr, bx, max_count, any, mode, seed, offset);
}

template <bool U8>
void launch_input_collate(dim3 grid, hipStream_t s, const void* x, float* out, int CH, int H, int W, const EraseCh& nc, const int4* mix,
                          const int4* bx, int max_count, int mode, unsigned long long seed, unsigned long long offset) {
#define GA_COLLATE_LAUNCH(MAXC) \
    hipLaunchKernelGGL((input_collate_kernel<U8, MAXC>), grid, dim3(256), 0, s, x, out, CH, H, W, nc, mix, bx, max_count, mode, seed, offset)
    switch (max_count) {
        case 1: GA_COLLATE_LAUNCH(1); break;
        case 2: GA_COLLATE_LAUNCH(2); break;
        case 3: GA_COLLATE_LAUNCH(3); break;
        case 4: GA_COLLATE_LAUNCH(4); break;
        default: GA_COLLATE_LAUNCH(0); break;               // 0: no boxes (the loop over them is empty); > 4: the generic loop
    }
#undef GA_COLLATE_LAUNCH
}

// dense target of per-sample lams (timm mixup_target with a lam vector): row b = y1 * lam[b] + y2 * (1 - lam[b]), y2 from
// target[B-1-b]; the complement, the two products and the sum are separate fp32 roundings, as the torch expression evaluates them
__global__ __launch_bounds__(256) void mixup_target_elem_kernel(const int64_t* __restrict__ t, float* __restrict__ out, int B, int NC,
                                                                const float* __restrict__ lam, float on, float off) {
    const long n = (long)B * NC;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int b = (int)(i / NC), c = (int)(i - (long)b * NC);
        const float y1 = c == (int)t[b] ? on : off, y2 = c == (int)t[B - 1 - b] ? on : off;
        const float l = lam[b];
        out[i] = blend_rn(y1, y2, l, 1.0f - l);
    }
}
}  // namespace

extern "C" int ga_input_erase(const void* x, int x_is_u8, float* out, int B, int CH, int H, int W, const float* mean, const float* std,
                              const int32_t* boxes, int max_count, int mode, uint64_t seed, uint64_t offset, ga_stream_t stream) {
    GA_REQUIRE(x && out && x != (const void*)out && B > 0 && B <= 65535 && CH > 0 && CH <= 4 && H > 0 && W > 0,
               "ga_input_erase: bad args (out of place, at most 4 channels, B <= 65535)");
    GA_REQUIRE(!x_is_u8 || (mean && std), "ga_input_erase: uint8 input needs mean / std");
    GA_REQUIRE(max_count >= 0 && (max_count == 0 || boxes) && mode >= 0 && mode <= 2 && (offset >> 63) == 0,
               "ga_input_erase: bad box table, mode (0 const, 1 rand, 2 pixel) or offset (< 2^63)");
    GA_REQUIRE((long)CH * H * W < (1l << 30), "ga_input_erase: a sample of 2^30 or more elements");
    GA_REQUIRE(((long)H * W) % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & (x_is_u8 ? 3 : 15)) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(boxes) & 15) == 0,
               "ga_input_erase: H*W must be a multiple of 4 and the buffers 4 / 16-byte aligned");
    EraseCh nc;
    for (int c = 0; c < 4; ++c) {
        nc.mean[c] = (x_is_u8 && c < CH) ? mean[c] : 0.f;     // host arrays
        nc.std[c] = (x_is_u8 && c < CH) ? std[c] : 1.f;
    }
    const long groups = (long)CH * H * W / 4;
    const int gx = (int)std::max<long>(1, std::min<long>((groups + 255) / 256, std::max<long>(1, 8192 / B)));
    const int4* bx = reinterpret_cast<const int4*>(boxes);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (x_is_u8)
        launch_input_erase<true>(dim3(gx, B), s, x, out, CH, H, W, nc, bx, max_count, mode, seed, offset);
    else
        launch_input_erase<false>(dim3(gx, B), s, x, out, CH, H, W, nc, bx, max_count, mode, seed, offset);
    return ga_check_launch("ga_input_erase");
}

extern "C" int ga_input_collate(const void* x, int x_is_u8, float* out, int B, int CH, int H, int W, const float* mean, const float* std,
                                const int32_t* mix, const int32_t* boxes, int max_count, int mode, uint64_t seed, uint64_t offset,
                                ga_stream_t stream) {
    GA_REQUIRE(x && out && x != (const void*)out && B > 0 && B <= 65535 && CH > 0 && CH <= 4 && H > 0 && W > 0,
               "ga_input_collate: bad args (out of place, at most 4 channels, B <= 65535)");
    GA_REQUIRE(B % 2 == 0 && mix, "ga_input_collate: the partner of sample b is B-1-b: B must be even; one mix row per sample");
    GA_REQUIRE(!x_is_u8 || (mean && std), "ga_input_collate: uint8 input needs mean / std");
    GA_REQUIRE(max_count >= 0 && (max_count == 0 || boxes) && mode >= 0 && mode <= 2 && (offset >> 63) == 0,
               "ga_input_collate: bad box table, mode (0 const, 1 rand, 2 pixel) or offset (< 2^63)");
    GA_REQUIRE((long)CH * H * W < (1l << 30), "ga_input_collate: a sample of 2^30 or more elements");
    GA_REQUIRE(((long)H * W) % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & (x_is_u8 ? 3 : 15)) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(mix) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(boxes) & 15) == 0,
               "ga_input_collate: H*W must be a multiple of 4, x 4 (uint8) / 16-byte aligned, out / mix / boxes 16-byte aligned");
    EraseCh nc;
    for (int c = 0; c < 4; ++c) {
        nc.mean[c] = (x_is_u8 && c < CH) ? mean[c] : 0.f;     // host arrays
        nc.std[c] = (x_is_u8 && c < CH) ? std[c] : 1.f;
    }
    if (!boxes) max_count = 0;                                 // boxes NULL / max_count 0: no erase
    const long groups = (long)CH * H * W / 4;
    const int gx = (int)std::max<long>(1, std::min<long>((groups + 255) / 256, std::max<long>(1, 8192 / B)));
    const int4* mx = reinterpret_cast<const int4*>(mix);
    const int4* bx = reinterpret_cast<const int4*>(boxes);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (x_is_u8)
        launch_input_collate<true>(dim3(gx, B), s, x, out, CH, H, W, nc, mx, bx, max_count, mode, seed, offset);
    else
        launch_input_collate<false>(dim3(gx, B), s, x, out, CH, H, W, nc, mx, bx, max_count, mode, seed, offset);
    return ga_check_launch("ga_input_collate");
}

extern "C" int ga_mixup_target_elem(const int64_t* target, float* out, int B, int NC, const float* lam, double smoothing,
                                    ga_stream_t stream) {
    GA_REQUIRE(target && out && lam && B > 0 && B % 2 == 0 && NC > 0, "ga_mixup_target_elem: bad args (B even, lam: device fp32 [B])");
    const long n = (long)B * NC;
    const int blocks = (int)std::max<long>(1, std::min<long>(4096, (n + 255) / 256));
    hipLaunchKernelGGL(mixup_target_elem_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), target, out, B, NC, lam,
                       (float)(1.0 - smoothing + smoothing / NC), (float)(smoothing / NC));
    return ga_check_launch("ga_mixup_target_elem");
}
