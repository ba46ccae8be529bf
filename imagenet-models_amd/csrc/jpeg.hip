// Baseline JPEG into the device input stage: the decoder that plugs in ahead of ga_resize_crop.  The host stage (jpeg_host.h, plain
// C++: ga_jpeg_probe / ga_jpeg_entropy_decode) turns a file into QUANTISED coefficients; this file rebuilds the pixels from them with
// libjpeg-turbo's default decode arithmetic restated (include/gaext.h states it; tests/_jpeg_ref.py restates it in numpy and is
// itself gated on PIL's bytes), writing the interleaved HWC images of a RaggedBatch.
//
// Two launches, one 64-byte table row per image, wave-uniform in each (blockIdx.y = image, scalar loads):
//   jpeg_idct_kernel    eight lanes per 8 x 8 block, 32 blocks per workgroup pass.  Lane r loads row r of the block -- 16 bytes, so a
//                       wave reads 1 KiB of coefficients in one instruction -- and dequantises it; the block goes through LDS to
//                       turn rows into columns, the column pass runs one column per lane, LDS turns it back, the row pass runs
//                       one row per lane and each lane stores its 8 bytes of the component's plane (8 lanes of a block row of the
//                       image side by side: 64-byte runs).  The planes are one byte per coefficient over the MCU-padded grid.
//   jpeg_colour_kernel  four consecutive pixels of the image's unpadded HWC byte string per thread = three aligned 4-byte stores, a
//                       wave writes 768 contiguous bytes; the chroma is upsampled where it is read (libjpeg's "fancy" triangle
//                       filters, its replicating ones for planes of at most two columns), then YCbCr -> RGB.
// Every intermediate of the IDCT is 64-bit: with int16 coefficients and 16-bit tables the dequantised value reaches 2^31, the
// column pass 2^38 and the row pass 2^56 (the bound is written at idct_1d); libjpeg computes in 64-bit longs too.  The kernels are
// far from compute bound either way (profiles/jpeg_decode_trace.md).  No atomics; the result does not depend on the launch shape.
#include "common.h"
#include "jpeg_host.h"

#include <algorithm>

namespace {
struct JpRow {
    int64_t coef_off;       // int16 units into coef: Y blocks [bh][bw][64], then Cb, then Cr
    int64_t dst_off;        // bytes into dst
    int64_t work_off;       // bytes into work: the planes in the same order, one byte per coefficient
    int32_t qt_off;         // uint16 units into qt: three tables of 64, natural order
    int32_t width, height;
    int32_t ncomp;          // 1 (grey: Y to all three channels) or 3 (YCbCr, chroma sampled 1 x 1)
    int32_t hs, vs;         // luma sampling: 1 x 1, 2 x 1 or 2 x 2
    int32_t mcus_w, mcus_h;
    int32_t pad[2];
};
static_assert(sizeof(JpRow) == 64, "one table row is 64 bytes");

constexpr int JP_MAX_EXTENT = ga_jpeg::MAX_EXTENT;
constexpr int JP_SLOTS = 32;            // blocks per workgroup pass (256 threads / 8 lanes)
constexpr int JP_LDS_BLOCK = 72;        // int64 words per block in LDS: 64 + 8, so that the four blocks of a half-wave start 16 banks apart

__host__ __device__ inline long jp_luma_blocks(const JpRow& r) { return (long)r.mcus_w * r.hs * r.mcus_h * r.vs; }
__host__ __device__ inline long jp_chroma_blocks(const JpRow& r) { return r.ncomp == 3 ? (long)r.mcus_w * r.mcus_h : 0; }
__host__ __device__ inline long jp_blocks(const JpRow& r) { return jp_luma_blocks(r) + 2 * jp_chroma_blocks(r); }

// jidctint.c "islow", one 1-D pass.  Bound, term by term with |in| <= M: t0, t1 <= 16384 M, t2 <= 24003 M, t3 <= 15136 M, so
// t10 .. t13 <= 40387 M; z5 <= 38532 M, z3 <= 70670 M, z4 <= 44924 M, z1 <= 14746 M, z2 <= 41990 M, so a0 .. a3 <= 137832 M; every sum
// before the shift is below 178219 M < 2^18 M.  The column pass sees M = 2^15 * 2^16 = 2^31 (int16 x uint16) -> below 2^49, its
// output >> 11 below 2^38 -> the row pass stays below 2^56: int64 never overflows.  int32 would, on values a file can hold: a
// dequantised +-2047 x 255 is 2^19, and 2^19 * 2^18 passes 2^31 in the column pass already.
__device__ __forceinline__ void idct_1d(long long v[8], int s) {
    const long long i0 = v[0], i1 = v[1], i2 = v[2], i3 = v[3], i4 = v[4], i5 = v[5], i6 = v[6], i7 = v[7];
    long long z1 = (i2 + i6) * 4433;
    const long long t2 = z1 - i6 * 15137, t3 = z1 + i2 * 6270;
    const long long t0 = (i0 + i4) * 8192, t1 = (i0 - i4) * 8192;
    const long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    long long a0 = i7, a1 = i5, a2 = i3, a3 = i1;
    z1 = a0 + a3;
    long long z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const long long z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    const long long h = 1ll << (s - 1);
    v[0] = (t10 + a3 + h) >> s; v[7] = (t10 - a3 + h) >> s;
    v[1] = (t11 + a2 + h) >> s; v[6] = (t11 - a2 + h) >> s;
    v[2] = (t12 + a1 + h) >> s; v[5] = (t12 - a1 + h) >> s;
    v[3] = (t13 + a0 + h) >> s; v[4] = (t13 - a0 + h) >> s;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpRow* __restrict__ rows, const int16_t* __restrict__ coef,
                                                        const uint16_t* __restrict__ qt, unsigned char* __restrict__ work) {
    __shared__ long long lds[JP_SLOTS * JP_LDS_BLOCK];
    const JpRow r = rows[blockIdx.y];
    // extents below 32768: at most 4096 x 4096 luma blocks, 1.5 times that in all -- block indices are ints (32-bit divisions)
    const int nb0 = (int)jp_luma_blocks(r), nbc = (int)jp_chroma_blocks(r), nblk = nb0 + 2 * nbc;
    const int lane = threadIdx.x & 7, slot = threadIdx.x >> 3;
    long long* __restrict__ mine = lds + slot * JP_LDS_BLOCK;
    // the trip count is the workgroup's, not the thread's: the barriers are reached by all
    for (int base = blockIdx.x * JP_SLOTS; base < nblk; base += gridDim.x * JP_SLOTS) {
        const int g = base + slot;                        // the image's blocks are consecutive in coef: Y, Cb, Cr
        const bool live = g < nblk;
        const int comp = g < nb0 ? 0 : (g - nb0 < nbc ? 1 : 2);
        long long v[8];
        if (live) {
            const uint4 c = *reinterpret_cast<const uint4*>(coef + r.coef_off + (long)g * 64 + lane * 8);
            const uint4 q = *reinterpret_cast<const uint4*>(qt + r.qt_off + comp * 64 + lane * 8);
            const unsigned cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[2 * i] = (long long)(short)(cw[i] & 0xffffu) * (long long)(qw[i] & 0xffffu);
                v[2 * i + 1] = (long long)(short)(cw[i] >> 16) * (long long)(qw[i] >> 16);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) mine[lane * 8 + i] = v[i];
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = mine[k * 8 + lane];          // column `lane`
            idct_1d(v, 11);
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int k = 0; k < 8; ++k) mine[k * 8 + lane] = v[k];
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = mine[lane * 8 + i];          // row `lane`
            idct_1d(v, 18);
            unsigned lo = 0u, hi = 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const long long x = v[i] + 128;
                const unsigned b = (unsigned)(x < 0 ? 0 : (x > 255 ? 255 : x));
                if (i < 4) lo |= b << (8 * i); else hi |= b << (8 * (i - 4));
            }
            const int local = comp == 0 ? g : g - nb0 - (comp - 1) * nbc;
            const int bw = comp == 0 ? r.mcus_w * r.hs : r.mcus_w;
            const int by = local / bw, bx = local - by * bw;
            unsigned char* plane = work + r.work_off + (comp == 0 ? 0l : ((long)nb0 + (long)(comp - 1) * nbc) * 64);
            *reinterpret_cast<uint2*>(plane + ((long)by * 8 + lane) * (8l * bw) + bx * 8) = make_uint2(lo, hi);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int jp_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the chroma sample of pixel (y, x): libjpeg's upsamplers evaluated at one output position.  cw x ch: the plane cropped to
// ceil(W / 2) x ceil(H / vs) -- the neighbours clamp there, not at the padded grid
__device__ __forceinline__ int jp_chroma(const unsigned char* __restrict__ p, long pitch, int cw, int ch, int hs, int vs, int y, int x) {
    if (hs == 1) return p[y * pitch + x];
    const int c = x >> 1, odd = x & 1;
    if (cw <= 2) return p[(vs == 2 ? y >> 1 : y) * pitch + c];            // h2v1_upsample / h2v2_upsample: replication
    const int nb = odd ? (c + 1 < cw ? c + 1 : c) : (c > 0 ? c - 1 : c);
    if (vs == 1) return (3 * p[y * pitch + c] + p[y * pitch + nb] + (odd ? 2 : 1)) >> 2;
    const int rr = y >> 1;
    const int nr = (y & 1) ? (rr + 1 < ch ? rr + 1 : rr) : (rr > 0 ? rr - 1 : rr);
    const unsigned char* __restrict__ a = p + rr * pitch;
    const unsigned char* __restrict__ b = p + nr * pitch;
    const int cs = 3 * a[c] + b[c], ns = 3 * a[nb] + b[nb];
    return (3 * cs + ns + (odd ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const JpRow* __restrict__ rows, const unsigned char* __restrict__ work,
                                                          unsigned char* __restrict__ dst) {
    const JpRow r = rows[blockIdx.y];
    const int W = r.width, H = r.height;
    const int npix = W * H, nquad = (npix + 3) / 4;             // extents below 32768: below 2^30, 32-bit divisions
    const long nb0 = jp_luma_blocks(r), nbc = jp_chroma_blocks(r);
    const unsigned char* __restrict__ yp = work + r.work_off;
    const unsigned char* __restrict__ cbp = yp + nb0 * 64;
    const unsigned char* __restrict__ crp = cbp + nbc * 64;
    const long ypitch = 8l * r.mcus_w * r.hs, cpitch = 8l * r.mcus_w;
    const int cw = (W + r.hs - 1) / r.hs, ch = (H + r.vs - 1) / r.vs;
    unsigned char* __restrict__ out = dst + r.dst_off;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < nquad; q += gridDim.x * 256) {
        const int p0 = q * 4;
        int y = p0 / W, x = p0 - y * W;
        const int cnt = npix - p0 < 4 ? npix - p0 : 4;
        unsigned char px[12];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e < cnt) {
                const int Y = yp[y * ypitch + x];
                int R = Y, G = Y, B = Y;
                if (r.ncomp == 3) {
                    const int cb = jp_chroma(cbp, cpitch, cw, ch, r.hs, r.vs, y, x) - 128;
                    const int cr = jp_chroma(crp, cpitch, cw, ch, r.hs, r.vs, y, x) - 128;
                    R = jp_clamp8(Y + ((91881 * cr + 32768) >> 16));
                    B = jp_clamp8(Y + ((116130 * cb + 32768) >> 16));
                    G = jp_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                }
                px[3 * e] = (unsigned char)R; px[3 * e + 1] = (unsigned char)G; px[3 * e + 2] = (unsigned char)B;
                if (++x == W) { x = 0; ++y; }
            } else {
                px[3 * e] = px[3 * e + 1] = px[3 * e + 2] = 0;
            }
        }
        unsigned char* o = out + 3l * p0;                    // 12 q behind a 16-byte aligned start
        if (cnt == 4) {
            unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                o4[k] = (unsigned)px[4 * k] | ((unsigned)px[4 * k + 1] << 8) | ((unsigned)px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
        } else {
            for (int k = 0; k < 3 * cnt; ++k) o[k] = px[k];  // the image's last bytes: nothing behind them is written
        }
    }
}

size_t jp_region_bytes(const JpRow& r) { return (size_t)jp_blocks(r) * 64; }

bool jp_row_shape_ok(const JpRow& r) {
    if (r.width < 1 || r.height < 1 || r.width >= JP_MAX_EXTENT || r.height >= JP_MAX_EXTENT) return false;
    if (!(r.ncomp == 1 || r.ncomp == 3)) return false;
    if (!((r.hs == 1 && r.vs == 1) || (r.ncomp == 3 && r.hs == 2 && (r.vs == 1 || r.vs == 2)))) return false;
    return r.mcus_w == (r.width + 8 * r.hs - 1) / (8 * r.hs) && r.mcus_h == (r.height + 8 * r.vs - 1) / (8 * r.vs);
}
}  // namespace

extern "C" int ga_jpeg_probe(const uint8_t* bytes, size_t n, int64_t* info) {
    GA_REQUIRE(bytes && info, "ga_jpeg_probe: bad args (bytes, info[24])");
    return ga_jpeg::probe(bytes, n, info);
}

extern "C" int ga_jpeg_entropy_decode(const uint8_t* bytes, size_t n, int16_t* coef, size_t coef_capacity, uint16_t* qt) {
    GA_REQUIRE(bytes && coef && qt, "ga_jpeg_entropy_decode: bad args (bytes, coef, qt[192])");
    return ga_jpeg::entropy_decode(bytes, n, coef, coef_capacity, qt);
}

extern "C" int ga_jpeg_check_table(const void* rows_host, int n_images, uint64_t coef_count, uint64_t qt_count, uint64_t work_bytes,
                                   uint64_t dst_bytes) {
    GA_REQUIRE(rows_host && n_images > 0 && n_images <= 65535, "ga_jpeg_check_table: bad args (a HOST table of 1 .. 65535 64-byte rows)");
    const JpRow* rows = reinterpret_cast<const JpRow*>(rows_host);
    for (int i = 0; i < n_images; ++i) {
        const JpRow& r = rows[i];
        GA_REQUIRE(jp_row_shape_ok(r),
                   "ga_jpeg_check_table: row %d is not a baseline image this path rebuilds (%d x %d, %d components, luma sampled %d x %d, "
                   "%d x %d MCUs: extents 1 .. 32767, 1 or 3 components, sampling 1x1 / 2x1 / 2x2, the MCU grid that covers the image)",
                   i, r.width, r.height, r.ncomp, r.hs, r.vs, r.mcus_w, r.mcus_h);
        const uint64_t ncoef = (uint64_t)jp_blocks(r) * 64;
        GA_REQUIRE(r.coef_off >= 0 && r.coef_off % 8 == 0 && (uint64_t)r.coef_off <= coef_count && ncoef <= coef_count - (uint64_t)r.coef_off,
                   "ga_jpeg_check_table: row %d has coefficients outside the buffer or off the 16-byte grid (offset %lld, %llu of %llu)", i,
                   (long long)r.coef_off, (unsigned long long)ncoef, (unsigned long long)coef_count);
        GA_REQUIRE(r.qt_off >= 0 && r.qt_off % 8 == 0 && (uint64_t)r.qt_off + 192 <= qt_count,
                   "ga_jpeg_check_table: row %d has its tables outside the buffer or off the 16-byte grid (offset %d, 192 of %llu)", i,
                   r.qt_off, (unsigned long long)qt_count);
        GA_REQUIRE(r.work_off >= 0 && r.work_off % 16 == 0 && (uint64_t)r.work_off <= work_bytes &&
                       jp_region_bytes(r) <= work_bytes - (uint64_t)r.work_off,
                   "ga_jpeg_check_table: row %d has its planes outside the workspace or off the 16-byte grid (offset %lld, %zu of %llu bytes)",
                   i, (long long)r.work_off, jp_region_bytes(r), (unsigned long long)work_bytes);
        GA_REQUIRE(r.dst_off >= 0 && r.dst_off % 16 == 0 && (uint64_t)r.dst_off <= dst_bytes &&
                       3ull * r.width * r.height <= dst_bytes - (uint64_t)r.dst_off,
                   "ga_jpeg_check_table: row %d has its image outside the destination or off the 16-byte grid (offset %lld, %d x %d x 3, "
                   "%llu bytes)", i, (long long)r.dst_off, r.height, r.width, (unsigned long long)dst_bytes);
    }
    return GA_OK;
}

extern "C" size_t ga_jpeg_work_bytes(const void* rows_host, int n_images) {
    if (!rows_host || n_images <= 0) return 0;
    const JpRow* rows = reinterpret_cast<const JpRow*>(rows_host);
    size_t total = 0;
    for (int i = 0; i < n_images; ++i) {
        if (!jp_row_shape_ok(rows[i])) return 0;
        total += jp_region_bytes(rows[i]);                   // a multiple of 64: regions laid back to back stay aligned
    }
    return total;
}

extern "C" int ga_jpeg_reconstruct(const void* table, int n_images, const int16_t* coef, const uint16_t* qt, void* work, void* dst,
                                   ga_stream_t stream) {
    GA_REQUIRE(table && coef && qt && work && dst && n_images > 0 && n_images <= 65535,
               "ga_jpeg_reconstruct: bad args (table, coef, qt, work and dst are device pointers, 1 <= n_images <= 65535)");
    GA_REQUIRE(((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(coef) | reinterpret_cast<uintptr_t>(qt) |
                 reinterpret_cast<uintptr_t>(work) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0,
               "ga_jpeg_reconstruct: table, coef, qt, work and dst must be 16-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const JpRow* tab = reinterpret_cast<const JpRow*>(table);
    // the images' sizes are known to the device only: a fixed number of workgroups per image strides over its blocks / pixels
    const int gx = (int)std::max<long>(1, std::min<long>(64, 16384 / n_images));
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(gx, n_images), dim3(256), 0, s, tab, coef, qt, reinterpret_cast<unsigned char*>(work));
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3(gx, n_images), dim3(256), 0, s, tab, (const unsigned char*)work,
                       reinterpret_cast<unsigned char*>(dst));
    return ga_check_launch("ga_jpeg_reconstruct");
}
