// timm RandAugment (`--aa rand-mN-mstd0.5-inc1`, every recipe of MAP/train_with_script.py:13-19) on the device, on the uint8 NCHW batch
// of timm's fast_collate, ahead of ga_input_collate / ga_input_erase / ga_u8_normalize.  The host (rand_augment.py) draws one 64-byte
// row per (sample, layer); this file applies it with the byte-exact arithmetic of the PIL calls timm makes (include/gaext.h states
// it; tests/_rand_augment_ref.py restates it in numpy and is itself gated on PIL's outputs).
//
// Per layer two launches, both with the row of a sample wave-uniform (scalar loads, one branch per workgroup):
//   ra_stats_kernel  grid (B), one workgroup per sample: only for autocontrast / equalize (three 256-bin integer LDS histograms
//                    -> three 256-byte LUTs) and contrast (integer sum of the grey image -> its rounded mean); every other kind
//                    returns at once.  Integer LDS atomics only: deterministic.
//   ra_apply_kernel  grid (x, B): four consecutive pixels per thread and channel, one 4-byte load and store each; the 3x3 and the
//                    gather ops read their neighbours as bytes from the (complete) previous layer.
// Layer l reads x (l = 0) or a ping-pong image in the caller's workspace and writes `out` (last layer) or the other image.
#include "common.h"

#include <algorithm>

namespace {
enum { RA_NONE, RA_AUTOCONTRAST, RA_EQUALIZE, RA_INVERT, RA_POSTERIZE, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_COLOR, RA_CONTRAST, RA_BRIGHTNESS,
       RA_SHARPNESS, RA_AFFINE, RA_KINDS };
enum { RA_NEAREST = 0, RA_BILINEAR = 2, RA_BICUBIC = 3 };

struct RaRow { int kind, interp, iarg; float farg; double m[6]; };
static_assert(sizeof(RaRow) == 64, "one table row is 64 bytes");
struct RaFill { unsigned c[3]; };

constexpr int RA_STATS_BYTES = 1024;     // per sample: lut[3][256], then the int mean of the grey image at byte 768

__device__ __forceinline__ unsigned gray_px(unsigned r, unsigned g, unsigned b) { return (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16; }

// PIL ImagingBlend: d + f * (a - d) in fp32, the product and the sum separately rounded (hipcc would contract them into an FMA);
// <= 0 -> 0, >= 255 -> 255, else truncated
__device__ __forceinline__ unsigned blend_px(float d, float a, float f) {
#pragma clang fp contract(off)
    const float t = f * (a - d);
    const float v = d + t;
    return v <= 0.f ? 0u : (v >= 255.f ? 255u : (unsigned)v);
}

__device__ __forceinline__ unsigned clip_trunc(double v) { return v <= 0.0 ? 0u : (v >= 255.0 ? 255u : (unsigned)v); }

__device__ __forceinline__ unsigned byte_of(unsigned w, int e) { return (w >> (8 * e)) & 255u; }

__device__ __forceinline__ unsigned load_word(const unsigned char* p) { return *reinterpret_cast<const unsigned*>(p); }

__global__ __launch_bounds__(1024) void ra_stats_kernel(const unsigned char* __restrict__ src, const RaRow* __restrict__ ops, int layer,
                                                        int n_layers, unsigned char* __restrict__ stats, int HW) {
    const int b = blockIdx.x, t = threadIdx.x;
    const int kind = ops[(long)b * n_layers + layer].kind;
    if (kind != RA_AUTOCONTRAST && kind != RA_EQUALIZE && kind != RA_CONTRAST) return;
    __shared__ unsigned hist[3 * 256];
    __shared__ unsigned long long gsum;
    __shared__ int lo[3], hi[3];
    const unsigned char* __restrict__ a = src + (long)b * 3 * HW;
    unsigned char* __restrict__ st = stats + (long)b * RA_STATS_BYTES;
    if (kind == RA_CONTRAST) {
        if (t == 0) gsum = 0ull;
        __syncthreads();
        unsigned long long s = 0ull;
        for (int p = t * 4; p < HW; p += 4096) {
            const unsigned r = load_word(a + p), g = load_word(a + HW + p), bl = load_word(a + 2 * HW + p);
#pragma unroll
            for (int e = 0; e < 4; ++e) s += gray_px(byte_of(r, e), byte_of(g, e), byte_of(bl, e));
        }
        atomicAdd(&gsum, s);                                   // integer: the order of the additions does not matter
        __syncthreads();
        if (t == 0) *reinterpret_cast<int*>(st + 768) = (int)((double)gsum / (double)HW + 0.5);     // ImageStat mean, int(mean + 0.5)
        return;
    }
    if (t < 768) hist[t] = 0u;
    __syncthreads();
    for (int p = t * 4; p < 3 * HW; p += 4096) {
        const unsigned w = load_word(a + p);
        unsigned* h = hist + (p / HW) * 256;                   // HW % 4 == 0: a word never spans two channels
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(&h[byte_of(w, e)], 1u);
    }
    __syncthreads();
    if (kind == RA_AUTOCONTRAST) {
        if (t < 3) {
            int l = 0, h = 255;
            while (l < 255 && hist[t * 256 + l] == 0u) ++l;
            while (h > 0 && hist[t * 256 + h] == 0u) --h;
            lo[t] = l;
            hi[t] = h;
        }
        __syncthreads();
        if (t < 768) {
            const int c = t >> 8, i = t & 255;
            unsigned v = (unsigned)i;
            if (hi[c] > lo[c]) {
#pragma clang fp contract(off)
                const double scale = 255.0 / (double)(hi[c] - lo[c]);
                const double offset = -(double)lo[c] * scale;
                const double r = (double)i * scale + offset;
                const int q = (int)r;                          // truncation toward zero, as Python's int()
                v = (unsigned)(q < 0 ? 0 : (q > 255 ? 255 : q));
            }
            st[t] = (unsigned char)v;
        }
        return;
    }
    // equalize: one thread per channel walks its 256 bins
    if (t < 3) {
        const unsigned* h = hist + t * 256;
        int nz = 0, last = 0;
        unsigned long long total = 0ull;
        for (int i = 0; i < 256; ++i)
            if (h[i]) { ++nz; last = i; total += h[i]; }
        const unsigned long long step = nz > 1 ? (total - h[last]) / 255ull : 0ull;
        unsigned long long n = step / 2ull;
        for (int i = 0; i < 256; ++i) {
            unsigned v = (unsigned)i;
            if (step) {
                const unsigned long long q = n / step;
                v = q > 255ull ? 255u : (unsigned)q;
                n += h[i];
            }
            st[t * 256 + i] = (unsigned char)v;
        }
    }
}

// ---- the 3x3 and gather ops: one output byte of channel plane `a` ---------------------------------------------------------------
// ImageFilter.SMOOTH (1,1,1,1,5,1,1,1,1)/13 of an interior pixel: the fp32 sum (exact: integers), / 13, + 0.5, clipped, truncated
__device__ __forceinline__ float smooth_px(const unsigned char* __restrict__ a, int y, int x, int W) {
#pragma clang fp contract(off)
    const unsigned char* r0 = a + (long)(y - 1) * W + x;
    const unsigned char* r1 = r0 + W;
    const unsigned char* r2 = r1 + W;
    const float s = (float)((unsigned)r0[-1] + r0[0] + r0[1] + r1[-1] + 5u * r1[0] + r1[1] + r2[-1] + r2[0] + r2[1]);
    const float v = s / 13.0f + 0.5f;
    return v <= 0.f ? 0.f : (v >= 255.f ? 255.f : (float)(unsigned)v);
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ double lerp_d(double v1, double v2, double d) {
#pragma clang fp contract(off)
    return v1 + (v2 - v1) * d;
}

__device__ __forceinline__ double cubic_d(double v1, double v2, double v3, double v4, double d) {
#pragma clang fp contract(off)
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

// PIL's 16.16 fixed point of its NEAREST affine: floor(v * 65536 + 0.5)
__device__ __forceinline__ long long fix16(double v) {
#pragma clang fp contract(off)
    return (long long)floor(v * 65536.0 + 0.5);
}

struct RaGeo {               // what a NEAREST transform needs besides the matrix, formed once per thread
    bool axis;               // m1 == m3 == 0: PIL steps the coordinate by repeated double additions
    long long a0, a1, a2, a3, a4, a5;
};

__device__ __forceinline__ RaGeo make_geo(const RaRow& r) {
#pragma clang fp contract(off)
    RaGeo g;
    g.axis = r.m[1] == 0.0 && r.m[3] == 0.0;
    g.a0 = fix16(r.m[0]); g.a1 = fix16(r.m[1]); g.a3 = fix16(r.m[3]); g.a4 = fix16(r.m[4]);
    g.a2 = fix16(r.m[2] + r.m[0] * 0.5 + r.m[1] * 0.5);
    g.a5 = fix16(r.m[5] + r.m[3] * 0.5 + r.m[4] * 0.5);
    return g;
}

// o + k * step as PIL's ImagingScaleAffine forms it (k roundings), truncated: -1 outside [0, size)
__device__ __forceinline__ int stepped_coord(double o, double step, int k, int size) {
#pragma clang fp contract(off)
    for (int i = 0; i < k; ++i) o += step;
    return (o < 0.0 || !(o < (double)size)) ? -1 : (int)o;
}

// source of output pixel (y, x) under NEAREST -> flat index inside a plane, -1: fill
__device__ __forceinline__ long nearest_src(const RaRow& r, const RaGeo& g, int y, int x, int H, int W) {
#pragma clang fp contract(off)
    int xs, ys;
    if (g.axis) {
        xs = stepped_coord(r.m[2] + r.m[0] * 0.5, r.m[0], x, W);
        ys = stepped_coord(r.m[5] + r.m[4] * 0.5, r.m[4], y, H);
    } else {
        const long long xx = (g.a2 + g.a1 * y + g.a0 * x) >> 16, yy = (g.a5 + g.a4 * y + g.a3 * x) >> 16;
        xs = (xx >= 0 && xx < W) ? (int)xx : -1;
        ys = (yy >= 0 && yy < H) ? (int)yy : -1;
    }
    return (xs < 0 || ys < 0) ? -1l : (long)ys * W + xs;
}

// the three channels of output pixel (y, x) under BILINEAR / BICUBIC, all in double (PIL's affine_transform + *_filter32RGB)
template <bool CUBIC>
__device__ __forceinline__ bool resample_px(const unsigned char* __restrict__ a, const RaRow& r, int y, int x, int H, int W, long HW,
                                            unsigned v[3]) {
#pragma clang fp contract(off)
    const double xc = (double)x + 0.5, yc = (double)y + 0.5;
    double xin = r.m[0] * xc + r.m[1] * yc + r.m[2];
    double yin = r.m[3] * xc + r.m[4] * yc + r.m[5];
    if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) return false;
    xin -= 0.5;
    yin -= 0.5;
    const double fx = floor(xin), fy = floor(yin);
    const double dx = xin - fx, dy = yin - fy;
    const int x0 = (int)fx, y0 = (int)fy;                      // -1 .. W-1 / H-1: every neighbour index is clamped to the image
    if (!CUBIC) {
        const int xa = clampi(x0, W - 1), xb = clampi(x0 + 1, W - 1);
        const long ra = (long)clampi(y0, H - 1) * W, rb = (long)clampi(y0 + 1, H - 1) * W;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned char* p = a + c * HW;
            const double t0 = lerp_d((double)p[ra + xa], (double)p[ra + xb], dx);
            const double t1 = lerp_d((double)p[rb + xa], (double)p[rb + xb], dx);
            v[c] = clip_trunc(lerp_d(t0, t1, dy));
        }
    } else {
        int xi[4];
        long ri[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            xi[k] = clampi(x0 - 1 + k, W - 1);
            ri[k] = (long)clampi(y0 - 1 + k, H - 1) * W;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned char* p = a + c * HW;
            double t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                t[k] = cubic_d((double)p[ri[k] + xi[0]], (double)p[ri[k] + xi[1]], (double)p[ri[k] + xi[2]], (double)p[ri[k] + xi[3]], dx);
            v[c] = clip_trunc(cubic_d(t[0], t[1], t[2], t[3], dy));
        }
    }
    return true;
}

// one sample, one layer, a compile-time KIND: the branch on the kind is taken once per workgroup (ra_apply_kernel)
template <int KIND>
__device__ __forceinline__ void apply_sample(const unsigned char* __restrict__ a, unsigned char* __restrict__ o, const RaRow& r,
                                             const unsigned char* __restrict__ st, int H, int W, const RaFill& fill,
                                             const unsigned char* lut) {
    const int HW = H * W;
    const float f = r.farg;
    const int iarg = r.iarg;
    const unsigned pmask = iarg >= 8 ? 255u : (~((1u << (8 - (iarg < 0 ? 0 : iarg))) - 1u)) & 255u;
    float mean = 0.f;
    if (KIND == RA_CONTRAST) mean = (float)*reinterpret_cast<const int*>(st + 768);
    RaGeo geo;
    if (KIND == RA_AFFINE) geo = make_geo(r);
    for (int p = (blockIdx.x * 256 + threadIdx.x) * 4; p < HW; p += gridDim.x * 1024) {
        unsigned w[3] = {0u, 0u, 0u}, res[3] = {0u, 0u, 0u};
        if (KIND != RA_AFFINE) {
#pragma unroll
            for (int c = 0; c < 3; ++c) w[c] = load_word(a + (long)c * HW + p);
        }
        if (KIND == RA_NONE) {
#pragma unroll
            for (int c = 0; c < 3; ++c) res[c] = w[c];
        } else if (KIND == RA_INVERT) {
#pragma unroll
            for (int c = 0; c < 3; ++c) res[c] = ~w[c];
        } else if (KIND == RA_POSTERIZE) {
#pragma unroll
            for (int c = 0; c < 3; ++c) res[c] = w[c] & (pmask * 0x01010101u);
        } else {
            int y = p / W, x = p - y * W;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (x >= W) { x -= W; ++y; }                   // H*W % 4 == 0, W itself need not be: a group may run into the next row
                unsigned v[3];
                const unsigned s0 = byte_of(w[0], e), s1 = byte_of(w[1], e), s2 = byte_of(w[2], e);
                if (KIND == RA_AUTOCONTRAST || KIND == RA_EQUALIZE) {
                    v[0] = lut[s0]; v[1] = lut[256 + s1]; v[2] = lut[512 + s2];
                } else if (KIND == RA_SOLARIZE) {
                    v[0] = (int)s0 < iarg ? s0 : 255u - s0; v[1] = (int)s1 < iarg ? s1 : 255u - s1; v[2] = (int)s2 < iarg ? s2 : 255u - s2;
                } else if (KIND == RA_SOLARIZE_ADD) {
                    const unsigned src[3] = {s0, s1, s2};
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int t = (int)src[c] + iarg;
                        v[c] = src[c] < 128u ? (unsigned)(t > 255 ? 255 : (t < 0 ? 0 : t)) : src[c];
                    }
                } else if (KIND == RA_COLOR) {
                    const float g = (float)gray_px(s0, s1, s2);
                    v[0] = blend_px(g, (float)s0, f); v[1] = blend_px(g, (float)s1, f); v[2] = blend_px(g, (float)s2, f);
                } else if (KIND == RA_CONTRAST) {
                    v[0] = blend_px(mean, (float)s0, f); v[1] = blend_px(mean, (float)s1, f); v[2] = blend_px(mean, (float)s2, f);
                } else if (KIND == RA_BRIGHTNESS) {
                    v[0] = blend_px(0.f, (float)s0, f); v[1] = blend_px(0.f, (float)s1, f); v[2] = blend_px(0.f, (float)s2, f);
                } else if (KIND == RA_SHARPNESS) {
                    const bool inner = y > 0 && y < H - 1 && x > 0 && x < W - 1;      // PIL copies the border row and column
                    const unsigned src[3] = {s0, s1, s2};
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float d = inner ? smooth_px(a + (long)c * HW, y, x, W) : (float)src[c];
                        v[c] = blend_px(d, (float)src[c], f);
                    }
                } else {                                        // RA_AFFINE
                    bool in;
                    if (r.interp == RA_BICUBIC) {
                        in = resample_px<true>(a, r, y, x, H, W, HW, v);
                    } else if (r.interp == RA_BILINEAR) {
                        in = resample_px<false>(a, r, y, x, H, W, HW, v);
                    } else {
                        const long s = nearest_src(r, geo, y, x, H, W);
                        in = s >= 0;
                        if (in) { v[0] = a[s]; v[1] = a[(long)HW + s]; v[2] = a[2l * HW + s]; }
                    }
                    if (!in) { v[0] = fill.c[0]; v[1] = fill.c[1]; v[2] = fill.c[2]; }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) res[c] |= (v[c] & 255u) << (8 * e);
                ++x;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<unsigned*>(o + (long)c * HW + p) = res[c];
    }
}

__global__ __launch_bounds__(256) void ra_apply_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                       const RaRow* __restrict__ ops, int layer, int n_layers,
                                                       const unsigned char* __restrict__ stats, int H, int W, RaFill fill) {
    const int b = blockIdx.y;
    const long per = 3l * H * W;
    const unsigned char* __restrict__ a = src + b * per;
    unsigned char* __restrict__ o = dst + b * per;
    const unsigned char* __restrict__ st = stats + (long)b * RA_STATS_BYTES;
    __shared__ unsigned char lut[768];
    RaRow r;
    r.kind = RA_NONE;
    if (ops) r = ops[(long)b * n_layers + layer];               // ops NULL: n_layers == 0, a copy
    if (r.kind == RA_AUTOCONTRAST || r.kind == RA_EQUALIZE) {
        for (int i = threadIdx.x; i < 768; i += 256) lut[i] = st[i];
        __syncthreads();
    }
    switch (r.kind) {
#define RA_CASE(K) case K: apply_sample<K>(a, o, r, st, H, W, fill, lut); break
        RA_CASE(RA_AUTOCONTRAST);
        RA_CASE(RA_EQUALIZE);
        RA_CASE(RA_INVERT);
        RA_CASE(RA_POSTERIZE);
        RA_CASE(RA_SOLARIZE);
        RA_CASE(RA_SOLARIZE_ADD);
        RA_CASE(RA_COLOR);
        RA_CASE(RA_CONTRAST);
        RA_CASE(RA_BRIGHTNESS);
        RA_CASE(RA_SHARPNESS);
        RA_CASE(RA_AFFINE);
#undef RA_CASE
        default: apply_sample<RA_NONE>(a, o, r, st, H, W, fill, lut); break;      // none, and every unknown kind
    }
}

size_t ra_image_bytes(int B, int CH, int H, int W) { return (((size_t)B * CH * H * W) + 255) & ~(size_t)255; }
int ra_images(int n_layers) { return n_layers >= 3 ? 2 : (n_layers == 2 ? 1 : 0); }
}  // namespace

extern "C" size_t ga_rand_augment_work_bytes(int B, int CH, int H, int W, int n_layers) {
    if (B <= 0 || CH <= 0 || H <= 0 || W <= 0 || n_layers < 0) return 0;
    return (size_t)B * RA_STATS_BYTES + (size_t)ra_images(n_layers) * ra_image_bytes(B, CH, H, W);
}

extern "C" int ga_rand_augment_check_table(const void* ops_host, int rows) {
    GA_REQUIRE(ops_host && rows >= 0, "ga_rand_augment_check_table: bad args (a HOST table of 64-byte rows)");
    const RaRow* r = reinterpret_cast<const RaRow*>(ops_host);
    for (int i = 0; i < rows; ++i) {
        GA_REQUIRE(r[i].kind >= 0 && r[i].kind < RA_KINDS, "ga_rand_augment_check_table: row %d has unknown kind %d (0 .. %d)", i, r[i].kind,
                   RA_KINDS - 1);
        GA_REQUIRE(r[i].interp == RA_NEAREST || r[i].interp == RA_BILINEAR || r[i].interp == RA_BICUBIC,
                   "ga_rand_augment_check_table: row %d has unknown interpolation %d (0 nearest, 2 bilinear, 3 bicubic)", i, r[i].interp);
    }
    return GA_OK;
}

extern "C" int ga_rand_augment(const void* x, void* out, void* work, size_t work_bytes, int B, int CH, int H, int W, const void* ops,
                               int n_layers, const uint8_t* fill, ga_stream_t stream) {
    GA_REQUIRE(x && out && x != (const void*)out && B > 0 && B <= 65535 && H > 0 && W > 0 && H < 32768 && W < 32768,
               "ga_rand_augment: bad args (out of place, B <= 65535, H and W below 32768)");
    GA_REQUIRE(CH == 3, "ga_rand_augment: CH must be 3 (the ops are PIL's on RGB images), got %d", CH);
    GA_REQUIRE(n_layers >= 0 && (n_layers == 0 || (ops && fill)), "ga_rand_augment: n_layers >= 0; a table and a fill colour for n_layers > 0");
    GA_REQUIRE((long)CH * H * W < (1l << 30), "ga_rand_augment: a sample of 2^30 or more elements");
    GA_REQUIRE(((long)H * W) % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(ops) & 15) == 0 && (reinterpret_cast<uintptr_t>(work) & 15) == 0,
               "ga_rand_augment: H*W must be a multiple of 4, x / out 4-byte aligned, ops / work 16-byte aligned");
    const size_t need = ga_rand_augment_work_bytes(B, CH, H, W, n_layers);
    GA_REQUIRE(n_layers == 0 || (work && work_bytes >= need), "ga_rand_augment: workspace of %zu bytes, %zu needed (ga_rand_augment_work_bytes)",
               work_bytes, need);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long groups = (long)H * W / 4;
    const int gx = (int)std::max<long>(1, std::min<long>((groups + 255) / 256, std::max<long>(1, 8192 / B)));
    RaFill fc = {{0u, 0u, 0u}};
    if (fill)
        for (int c = 0; c < 3; ++c) fc.c[c] = fill[c];          // a host array
    const unsigned char* src = reinterpret_cast<const unsigned char*>(x);
    unsigned char* stats = reinterpret_cast<unsigned char*>(work);
    unsigned char* img[2] = {nullptr, nullptr};
    if (n_layers > 0) {
        img[0] = stats + (size_t)B * RA_STATS_BYTES;
        img[1] = img[0] + ra_image_bytes(B, CH, H, W);
    }
    const RaRow* tab = reinterpret_cast<const RaRow*>(ops);
    if (n_layers == 0) {
        hipLaunchKernelGGL(ra_apply_kernel, dim3(gx, B), dim3(256), 0, s, src, reinterpret_cast<unsigned char*>(out), (const RaRow*)nullptr, 0,
                           0, (const unsigned char*)nullptr, H, W, fc);
        return ga_check_launch("ga_rand_augment");
    }
    for (int l = 0; l < n_layers; ++l) {
        unsigned char* dst = l == n_layers - 1 ? reinterpret_cast<unsigned char*>(out) : img[l & 1];
        hipLaunchKernelGGL(ra_stats_kernel, dim3(B), dim3(1024), 0, s, src, tab, l, n_layers, stats, H * W);
        hipLaunchKernelGGL(ra_apply_kernel, dim3(gx, B), dim3(256), 0, s, src, dst, tab, l, n_layers, (const unsigned char*)stats, H, W, fc);
        src = dst;
    }
    return ga_check_launch("ga_rand_augment");
}
