// The first step of every recipe's input stage on the device: timm's RandomResizedCropAndInterpolation + RandomHorizontalFlip
// (training) and Resize + CenterCrop (evaluation) of DECODED images -- one byte buffer of interleaved HWC RGB images of any sizes,
// back to back -- into the uint8 NCHW batch of timm's fast_collate, ahead of ga_rand_augment / ga_input_collate / ga_input_erase /
// ga_u8_normalize.  The host (resize_crop.py) draws one 64-byte row per sample; this file applies it with the byte-exact integer
// arithmetic of PIL's ImagingResample for 8-bit channels (include/gaext.h states it; tests/_resize_crop_ref.py restates it in numpy
// and is itself gated on PIL's outputs).
//
// Four launches, the row of a sample wave-uniform in each (blockIdx.y = sample, scalar loads):
//   rc_layout_kernel  one workgroup: the prefix sum of the samples' workspace regions -> int64 off[B + 1] at the head of `work`
//   rc_coeff_kernel   grid (x, B): one thread per output column and per output row of the WINDOW: its (xmin, count) and its integer
//                     coefficients, by rs_column() -- the device function ga_resample_coeffs exposes -- into the sample's region,
//                     tap-major ([k][column]) so that the passes read them coalesced
//   rc_hpass_kernel   grid (x, B): box rows -> planar [3][h][OW] bytes in the region; one output column and four consecutive box rows
//                     per thread, neighbouring lanes on neighbouring columns; the taps are loops over the box rows' interleaved
//                     bytes (byte loads: a row pitch of 3 * src_w has no alignment), the flip and the window's column offset are
//                     folded into the column index
//   rc_vpass_kernel   grid (x, B): reads the planar rows as 4-byte words, coalesced along OW, four output pixels per thread and channel
// Tap loops are loops: no cap on the scale factor, no LDS tile.  No atomics; the result does not depend on the launch shape.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace {
enum { RS_BILINEAR = 2, RS_BICUBIC = 3 };
constexpr int RS_PRECISION_BITS = 22;
constexpr int RS_MAX_EXTENT = 32768;        // every extent is below this

struct RcRow {
    int64_t src_off;
    int src_h, src_w;
    int top, left, h, w;
    int vh, vw;
    int oy, ox;
    int interp, flip;
    int pad[2];
};
static_assert(sizeof(RcRow) == 64, "one table row is 64 bytes");

__host__ __device__ inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// the most taps one output index can have: PIL's ksize = (int)ceil(support) * 2 + 1, and never more than the input has
__host__ __device__ inline int rs_ksize_pil(int in, int out, int interp) {
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = (interp == RS_BILINEAR ? 1.0 : 2.0) * fs;
    return (int)ceil(support) * 2 + 1;
}
__host__ __device__ inline int rs_ksize(int in, int out, int interp) {
    const int k = rs_ksize_pil(in, out, interp);
    return k < in ? k : in;
}

// the workspace region of one sample: coefficients and bounds of the window's columns, of its rows, then the planar image
struct RcRegion { size_t coef_h, bnd_h, coef_v, bnd_v, img, total; int kh, kv; };
__host__ __device__ inline RcRegion rc_region(const RcRow& r, int OH, int OW) {
    RcRegion g;
    g.kh = rs_ksize(r.w, r.vw, r.interp);
    g.kv = rs_ksize(r.h, r.vh, r.interp);
    g.coef_h = 0;
    g.bnd_h = g.coef_h + align16((size_t)4 * g.kh * OW);
    g.coef_v = g.bnd_h + align16((size_t)8 * OW);
    g.bnd_v = g.coef_v + align16((size_t)4 * g.kv * OH);
    g.img = g.bnd_v + align16((size_t)8 * OH);
    g.total = g.img + align16((size_t)3 * r.h * OW);
    return g;
}
__host__ __device__ inline size_t rc_header_bytes(int B) { return align16((size_t)8 * ((size_t)B + 1)); }

// ---- PIL's filters and precompute_coeffs + normalize_coeffs_8bpc for ONE output index, all in double without contraction ---------
__device__ __forceinline__ double rs_bilinear(double t) {
#pragma clang fp contract(off)
    if (t < 0.0) t = -t;
    if (t < 1.0) return 1.0 - t;
    return 0.0;
}

__device__ __forceinline__ double rs_bicubic(double t) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (t < 0.0) t = -t;
    if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1;
    if (t < 2.0) return (((t - 5) * t + 8) * t - 4) * a;
    return 0.0;
}

template <bool CUBIC>
__device__ __forceinline__ double rs_weight(int x, double center, double ss) {
#pragma clang fp contract(off)
    const double t = (x - center + 0.5) * ss;
    return CUBIC ? rs_bicubic(t) : rs_bilinear(t);
}

// output index xx of an axis resized from `in` to `out`: coef[k * stride] for k < count, -> (xmin, count)
template <bool CUBIC>
__device__ __forceinline__ int2 rs_column_t(int in, int out, int xx, int* __restrict__ coef, long stride) {
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = (CUBIC ? 2.0 : 1.0) * fs;
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / fs;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int count = xmax - xmin;
    double ww = 0.0;
    for (int k = 0; k < count; ++k) ww += rs_weight<CUBIC>(k + xmin, center, ss);      // ascending, as PIL sums them
    for (int k = 0; k < count; ++k) {
        double w = rs_weight<CUBIC>(k + xmin, center, ss);
        if (ww != 0.0) w = w / ww;                                                     // a true division
        coef[k * stride] = w < 0 ? (int)(-0.5 + w * (double)(1 << RS_PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << RS_PRECISION_BITS));
    }
    return make_int2(xmin, count);
}

__device__ __forceinline__ int2 rs_column(int in, int out, int interp, int xx, int* __restrict__ coef, long stride) {
    return interp == RS_BICUBIC ? rs_column_t<true>(in, out, xx, coef, stride) : rs_column_t<false>(in, out, xx, coef, stride);
}

__device__ __forceinline__ unsigned rs_clip8(int acc) {
    const int v = acc >> RS_PRECISION_BITS;               // arithmetic
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---- ga_resample_coeffs ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rs_coeffs_kernel(int in, int out, int interp, int* __restrict__ bounds, int* __restrict__ coeffs,
                                                        int ksize) {
    const int xx = blockIdx.x * 256 + threadIdx.x;
    if (xx >= out) return;
    int* row = coeffs + (long)xx * ksize;
    const int2 b = rs_column(in, out, interp, xx, row, 1);
    for (int k = b.y; k < ksize; ++k) row[k] = 0;
    bounds[2 * xx] = b.x;
    bounds[2 * xx + 1] = b.y;
}

// ---- ga_resize_crop ----------------------------------------------------------------------------------------------------------------
// off[b] = byte offset of sample b's region in `work` (behind the header); off[B] = the bytes the table needs
__global__ __launch_bounds__(256) void rc_layout_kernel(const RcRow* __restrict__ rows, long long* __restrict__ off, int B, int OH, int OW) {
    __shared__ unsigned long long scan[256];
    __shared__ unsigned long long carry;
    const int t = threadIdx.x;
    if (t == 0) carry = rc_header_bytes(B);
    __syncthreads();
    for (int base = 0; base < B; base += 256) {
        const int b = base + t;
        const unsigned long long mine = b < B ? rc_region(rows[b], OH, OW).total : 0ull;
        scan[t] = mine;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const unsigned long long add = t >= d ? scan[t - d] : 0ull;
            __syncthreads();
            scan[t] += add;
            __syncthreads();
        }
        const unsigned long long c = carry;
        if (b < B) off[b] = (long long)(c + scan[t] - mine);
        __syncthreads();
        if (t == 255) carry = c + scan[255];
        __syncthreads();
    }
    if (t == 0) off[B] = (long long)carry;
}

__global__ __launch_bounds__(256) void rc_coeff_kernel(const RcRow* __restrict__ rows, unsigned char* __restrict__ work, size_t work_bytes,
                                                       int B, int OH, int OW) {
    const long long* off = reinterpret_cast<const long long*>(work);
    if ((size_t)off[B] > work_bytes) return;               // a workspace the table does not fit: nothing is written (wave-uniform)
    const int b = blockIdx.y;
    const RcRow r = rows[b];
    const RcRegion g = rc_region(r, OH, OW);
    unsigned char* reg = work + off[b];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < OW + OH; i += gridDim.x * 256) {
        if (i < OW) {                                       // column i of the window: resized column ox + i, mirrored under flip
            const int xx = r.flip ? r.vw - 1 - (r.ox + i) : r.ox + i;
            const int2 bd = rs_column(r.w, r.vw, r.interp, xx, reinterpret_cast<int*>(reg + g.coef_h) + i, OW);
            reinterpret_cast<int2*>(reg + g.bnd_h)[i] = bd;
        } else {
            const int j = i - OW;
            const int2 bd = rs_column(r.h, r.vh, r.interp, r.oy + j, reinterpret_cast<int*>(reg + g.coef_v) + j, OH);
            reinterpret_cast<int2*>(reg + g.bnd_v)[j] = bd;
        }
    }
}

__global__ __launch_bounds__(256) void rc_hpass_kernel(const unsigned char* __restrict__ src, const RcRow* __restrict__ rows,
                                                       unsigned char* __restrict__ work, size_t work_bytes, int B, int OH, int OW) {
    const long long* off = reinterpret_cast<const long long*>(work);
    if ((size_t)off[B] > work_bytes) return;
    const int b = blockIdx.y;
    const RcRow r = rows[b];
    const RcRegion g = rc_region(r, OH, OW);
    unsigned char* reg = work + off[b];
    const int* __restrict__ coef = reinterpret_cast<const int*>(reg + g.coef_h);
    const int2* __restrict__ bnd = reinterpret_cast<const int2*>(reg + g.bnd_h);
    unsigned char* __restrict__ img = reg + g.img;
    const unsigned char* __restrict__ box = src + r.src_off + ((long)r.top * r.src_w + r.left) * 3;
    const long pitch = 3l * r.src_w;
    const long plane = (long)r.h * OW;
    // one output column and four consecutive box rows per thread: neighbouring lanes take neighbouring columns, so a wave's
    // coefficient load is one contiguous run and its byte loads of a tap fall into a few cache lines; a coefficient is loaded once
    // for twelve multiply-adds
    const long items = (long)((r.h + 3) / 4) * OW;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
        const int yg = (int)(it / OW), j = (int)(it - (long)yg * OW);
        const int y0 = yg * 4;
        const int rows_here = r.h - y0 < 4 ? r.h - y0 : 4;
        const int2 bd = bnd[j];
        const unsigned char* __restrict__ p = box + y0 * pitch + 3l * bd.x;
        int acc[4][3];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[e][c] = 1 << (RS_PRECISION_BITS - 1);
        for (int k = 0; k < bd.y; ++k) {
            const int cf = coef[(long)k * OW + j];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e < rows_here) {                       // a row below the box is never read
                    const unsigned char* __restrict__ px = p + e * pitch + 3 * k;
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[e][c] += (int)px[c] * cf;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e < rows_here) {
#pragma unroll
                for (int c = 0; c < 3; ++c) img[c * plane + (long)(y0 + e) * OW + j] = (unsigned char)rs_clip8(acc[e][c]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void rc_vpass_kernel(const RcRow* __restrict__ rows, const unsigned char* __restrict__ work,
                                                       size_t work_bytes, unsigned char* __restrict__ out, int B, int OH, int OW) {
    const long long* off = reinterpret_cast<const long long*>(work);
    if ((size_t)off[B] > work_bytes) return;
    const int b = blockIdx.y;
    const RcRow r = rows[b];
    const RcRegion g = rc_region(r, OH, OW);
    const unsigned char* reg = work + off[b];
    const int* __restrict__ coef = reinterpret_cast<const int*>(reg + g.coef_v);
    const int2* __restrict__ bnd = reinterpret_cast<const int2*>(reg + g.bnd_v);
    const unsigned char* __restrict__ img = reg + g.img;
    unsigned char* __restrict__ o = out + (long)b * 3 * OH * OW;
    const int quads = OW / 4;
    const long plane = (long)r.h * OW;
    const long items = 3l * OH * quads;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
        const int q = (int)(it % quads);
        const int cy = (int)(it / quads);                   // c * OH + y
        const int c = cy / OH, y = cy - c * OH;
        const int2 bd = bnd[y];
        const unsigned char* __restrict__ p = img + c * plane + (long)bd.x * OW + q * 4;
        int a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = 1 << (RS_PRECISION_BITS - 1);
        for (int k = 0; k < bd.y; ++k) {
            const int cf = coef[(long)k * OH + y];
            const unsigned w = *reinterpret_cast<const unsigned*>(p + (long)k * OW);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] += (int)((w >> (8 * e)) & 255u) * cf;
        }
        unsigned res = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) res |= rs_clip8(a[e]) << (8 * e);
        *reinterpret_cast<unsigned*>(o + (long)cy * OW + q * 4) = res;
    }
}

// one row of a HOST table against its image, the output size and the source buffer
int rc_check_row(const RcRow& r, int i, int OH, int OW, uint64_t src_bytes) {
    GA_REQUIRE(r.src_h >= 1 && r.src_w >= 1 && r.src_h < RS_MAX_EXTENT && r.src_w < RS_MAX_EXTENT && r.vh >= 1 && r.vw >= 1 &&
                   r.vh < RS_MAX_EXTENT && r.vw < RS_MAX_EXTENT,
               "ga_resize_crop_check_table: row %d has an extent outside 1 .. 32767 (source %d x %d, resized %d x %d)", i, r.src_h, r.src_w,
               r.vh, r.vw);
    GA_REQUIRE(r.h >= 1 && r.w >= 1, "ga_resize_crop_check_table: row %d has an empty box (%d x %d)", i, r.h, r.w);
    GA_REQUIRE(r.top >= 0 && r.left >= 0 && (long)r.top + r.h <= r.src_h && (long)r.left + r.w <= r.src_w,
               "ga_resize_crop_check_table: row %d has a box outside its image (top %d left %d %d x %d in %d x %d)", i, r.top, r.left, r.h,
               r.w, r.src_h, r.src_w);
    GA_REQUIRE(r.src_off >= 0 && (uint64_t)r.src_off <= src_bytes && 3ull * r.src_h * r.src_w <= src_bytes - (uint64_t)r.src_off,
               "ga_resize_crop_check_table: row %d has an image outside the source buffer (offset %lld, %d x %d x 3, %llu bytes)", i,
               (long long)r.src_off, r.src_h, r.src_w, (unsigned long long)src_bytes);
    GA_REQUIRE(r.oy >= 0 && r.ox >= 0 && (long)r.oy + OH <= r.vh && (long)r.ox + OW <= r.vw,
               "ga_resize_crop_check_table: row %d has a window outside the resized image (oy %d ox %d %d x %d in %d x %d)", i, r.oy, r.ox,
               OH, OW, r.vh, r.vw);
    GA_REQUIRE(r.interp == RS_BILINEAR || r.interp == RS_BICUBIC,
               "ga_resize_crop_check_table: row %d has unknown interpolation %d (2 bilinear, 3 bicubic)", i, r.interp);
    GA_REQUIRE(r.flip == 0 || r.flip == 1, "ga_resize_crop_check_table: row %d has flip %d (0 or 1)", i, r.flip);
    return GA_OK;
}

int rc_check_shape(const char* who, int B, int OH, int OW) {
    GA_REQUIRE(B > 0 && B <= 65535 && OH >= 1 && OW >= 1 && OH < RS_MAX_EXTENT && OW < RS_MAX_EXTENT,
               "%s: bad args (1 <= B <= 65535, OH and OW in 1 .. 32767)", who);
    GA_REQUIRE(OW % 4 == 0, "%s: OW must be a multiple of 4 (four output pixels per store), got %d", who, OW);
    return GA_OK;
}

// the workspace of a table whose every box is one row high with one tap per axis: what any table needs at least
size_t rc_min_work_bytes(int B, int OH, int OW) {
    RcRow r = {};
    r.h = r.w = r.vh = r.vw = 1;
    r.interp = RS_BILINEAR;
    return rc_header_bytes(B) + (size_t)B * rc_region(r, OH, OW).total;
}
}  // namespace

extern "C" int ga_resize_crop_check_table(const void* rows_host, int B, int OH, int OW, uint64_t src_bytes) {
    GA_REQUIRE(rows_host, "ga_resize_crop_check_table: bad args (a HOST table of 64-byte rows)");
    if (int rc = rc_check_shape("ga_resize_crop_check_table", B, OH, OW)) return rc;
    const RcRow* r = reinterpret_cast<const RcRow*>(rows_host);
    for (int i = 0; i < B; ++i)
        if (int rc = rc_check_row(r[i], i, OH, OW, src_bytes)) return rc;
    return GA_OK;
}

extern "C" size_t ga_resize_crop_work_bytes(const void* rows_host, int B, int OH, int OW) {
    if (!rows_host || B <= 0 || OH <= 0 || OW <= 0) return 0;
    const RcRow* r = reinterpret_cast<const RcRow*>(rows_host);
    size_t total = rc_header_bytes(B);
    for (int i = 0; i < B; ++i) {
        if (r[i].h < 1 || r[i].w < 1 || r[i].vh < 1 || r[i].vw < 1) return 0;
        total += rc_region(r[i], OH, OW).total;
    }
    return total;
}

extern "C" int ga_resize_crop(const void* src, uint64_t src_bytes, const void* rows, void* out, void* work, size_t work_bytes, int B,
                              int OH, int OW, ga_stream_t stream) {
    GA_REQUIRE(src && rows && out && work && src_bytes > 0, "ga_resize_crop: bad args (src, rows, out and work are device pointers)");
    if (int rc = rc_check_shape("ga_resize_crop", B, OH, OW)) return rc;
    GA_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(work) & 15) == 0,
               "ga_resize_crop: out, rows and work must be 16-byte aligned");
    const size_t least = rc_min_work_bytes(B, OH, OW);
    GA_REQUIRE(work_bytes >= least, "ga_resize_crop: workspace of %zu bytes, at least %zu needed (ga_resize_crop_work_bytes of the table)",
               work_bytes, least);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const RcRow* tab = reinterpret_cast<const RcRow*>(rows);
    unsigned char* w = reinterpret_cast<unsigned char*>(work);
    hipLaunchKernelGGL(rc_layout_kernel, dim3(1), dim3(256), 0, s, tab, reinterpret_cast<long long*>(w), B, OH, OW);
    hipLaunchKernelGGL(rc_coeff_kernel, dim3((OW + OH + 255) / 256, B), dim3(256), 0, s, tab, w, work_bytes, B, OH, OW);
    // the box height is known to the device only: a fixed number of workgroups per sample strides over its rows
    const int gx = (int)std::max<long>(1, std::min<long>(64, 16384 / B));
    hipLaunchKernelGGL(rc_hpass_kernel, dim3(gx, B), dim3(256), 0, s, reinterpret_cast<const unsigned char*>(src), tab, w, work_bytes, B, OH,
                       OW);
    const long items = 3l * OH * (OW / 4);
    const int gv = (int)std::max<long>(1, std::min<long>((items + 255) / 256, std::max<long>(1, 16384 / B)));
    hipLaunchKernelGGL(rc_vpass_kernel, dim3(gv, B), dim3(256), 0, s, tab, (const unsigned char*)w, work_bytes,
                       reinterpret_cast<unsigned char*>(out), B, OH, OW);
    return ga_check_launch("ga_resize_crop");
}

extern "C" int ga_resample_coeffs(int in_size, int out_size, int interp, int32_t* bounds, int32_t* coeffs, int ksize, ga_stream_t stream) {
    GA_REQUIRE(bounds && coeffs && in_size >= 1 && out_size >= 1 && in_size < RS_MAX_EXTENT && out_size < RS_MAX_EXTENT,
               "ga_resample_coeffs: bad args (sizes in 1 .. 32767)");
    GA_REQUIRE(interp == RS_BILINEAR || interp == RS_BICUBIC, "ga_resample_coeffs: unknown interpolation %d (2 bilinear, 3 bicubic)", interp);
    GA_REQUIRE(ksize >= rs_ksize(in_size, out_size, interp), "ga_resample_coeffs: ksize %d, an output index has up to %d taps", ksize,
               rs_ksize(in_size, out_size, interp));
    GA_REQUIRE((reinterpret_cast<uintptr_t>(bounds) & 3) == 0 && (reinterpret_cast<uintptr_t>(coeffs) & 3) == 0,
               "ga_resample_coeffs: bounds and coeffs must be 4-byte aligned");
    hipLaunchKernelGGL(rs_coeffs_kernel, dim3((out_size + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), in_size, out_size,
                       interp, bounds, coeffs, ksize);
    return ga_check_launch("ga_resample_coeffs");
}
