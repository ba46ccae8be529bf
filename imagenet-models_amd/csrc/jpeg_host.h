// Host entropy stage of the JPEG decoder (include/gaext.h: ga_jpeg_probe / ga_jpeg_entropy_decode): marker parsing and baseline
// Huffman decoding into QUANTISED coefficients, in plain C++ -- no HIP, no allocation, no global state -- so that a stand-alone
// program (tools/jpeg_host_fuzz.cpp) compiles exactly this code under the host sanitizers.  csrc/jpeg.hip includes it and exports the
// two entry points; the pixel reconstruction (dequantise, IDCT, upsample, colour) is the device's.
//
// Rules this file keeps: every read is checked against the end of the input (Reader::n), every write against the capacity the caller
// gave; every loop runs over a count taken from a header field that was itself checked against the remaining input, or consumes
// input; arithmetic that can wrap is done unsigned.  What libjpeg would decode with a warning only (garbage before a restart marker,
// a run past coefficient 63, a scan that ends early) is CORRUPT here: PIL refuses truncated files, and a loader should not train on
// a half-grey image.  What is a valid JPEG of a kind the device path does not rebuild is UNSUPPORTED, never an error: the caller
// hands those to another decoder.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace ga_jpeg {

enum { OK = 0, UNSUPPORTED = 1, CORRUPT = 2 };
enum { INFO_LEN = 24, MAX_EXTENT = 32768 };        // every extent is below MAX_EXTENT (ga_resize_crop's limit)
// info[]: 0 width, 1 height, 2 components (1 or 3), 3 hmax, 4 vmax, 5 int16 coefficients of the whole image, 6 restart interval in
// MCUs (0: none), 7 MCUs per row, 8 MCU rows; component c: 9 + 4c .. 12 + 4c = h, v, blocks_w, blocks_h over the MCU-padded grid;
// 21 + c = where the component starts in the coefficient buffer (int16 units)

static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool defined;
    uint8_t bits[17];         // codes per length 1..16
    uint8_t vals[256];
    int nvals;
    // derived by derive(): a 9-bit look-ahead (length << 8 | symbol, 0: longer code) and the canonical ranges per length
    uint16_t look[512];
    int32_t maxcode[18];      // largest code of length l, -1 if none; [17] = sentinel
    int32_t valoff[17];       // vals index of the first code of length l minus that code
};

struct Component { int id, h, v, tq, td, ta; };

struct Header {
    int width, height, ncomp, hmax, vmax;
    int restart;                    // MCUs between restart markers, 0: none
    int mcus_w, mcus_h;
    Component comp[3];
    uint16_t qt[4][64];             // natural order
    bool qt_defined[4];
    Huff dc[4], ac[4];
    size_t scan;                    // first byte of the entropy-coded data
};

inline int derive(Huff& h) {
    int code = 0, k = 0;
    for (int i = 0; i < 512; ++i) h.look[i] = 0;
    for (int l = 1; l <= 16; ++l) {
        h.valoff[l] = k - code;
        if (h.bits[l]) {
            if (code + h.bits[l] > (1 << l)) return CORRUPT;          // more codes than the length has room for
            for (int i = 0; i < h.bits[l]; ++i, ++code, ++k) {
                if (l <= 9) {
                    const int lo = code << (9 - l), n = 1 << (9 - l);
                    for (int j = 0; j < n; ++j) h.look[lo + j] = (uint16_t)((l << 8) | h.vals[k]);
                }
            }
            h.maxcode[l] = code - 1;
        } else {
            h.maxcode[l] = -1;
        }
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    return OK;
}

inline unsigned be16(const uint8_t* p) { return ((unsigned)p[0] << 8) | p[1]; }

// markers up to and including SOS.  *scan_components: the Ns of SOS
inline int parse_header(const uint8_t* b, size_t n, Header& H) {
    memset(&H, 0, sizeof(H));
    if (!b || n < 4 || b[0] != 0xFF || b[1] != 0xD8) return n >= 2 && b && b[0] == 0xFF && b[1] == 0xD8 ? CORRUPT : UNSUPPORTED;
    bool jfif = false, adobe = false, sof = false;
    int adobe_transform = 0;
    size_t p = 2;
    for (;;) {
        // the next marker: 0xFF, any number of fill 0xFF, the code
        if (p >= n) return CORRUPT;
        if (b[p] != 0xFF) return CORRUPT;
        while (p < n && b[p] == 0xFF) ++p;
        if (p >= n) return CORRUPT;
        const int m = b[p++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;      // parameterless
        if (m == 0xD9 || m == 0x00) return CORRUPT;                           // EOI ahead of a scan
        if (n - p < 2) return CORRUPT;
        const size_t len = be16(b + p);
        if (len < 2 || len > n - p) return CORRUPT;
        const uint8_t* s = b + p + 2;
        const size_t sl = len - 2;
        if (m == 0xC0 || m == 0xC1) {
            if (sof) return UNSUPPORTED;
            if (sl < 6) return CORRUPT;
            if (s[0] != 8) return UNSUPPORTED;                                 // 12-bit samples
            H.height = (int)be16(s + 1);
            H.width = (int)be16(s + 3);
            H.ncomp = s[5];
            if (H.ncomp != 1 && H.ncomp != 3) return UNSUPPORTED;
            if (sl != (size_t)6 + 3 * (size_t)H.ncomp) return CORRUPT;
            if (H.height < 1 || H.width < 1) return UNSUPPORTED;               // height 0: taken from a DNL marker
            if (H.height >= MAX_EXTENT || H.width >= MAX_EXTENT) return UNSUPPORTED;
            for (int c = 0; c < H.ncomp; ++c) {
                Component& k = H.comp[c];
                k.id = s[6 + 3 * c];
                k.h = s[7 + 3 * c] >> 4;
                k.v = s[7 + 3 * c] & 15;
                k.tq = s[8 + 3 * c];
                if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4) return CORRUPT;
                if (k.tq > 3) return CORRUPT;
            }
            sof = true;
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
            return UNSUPPORTED;                                                // progressive, lossless, differential, arithmetic, DAC
        } else if (m == 0xC4) {
            size_t q = 0;
            while (q < sl) {
                if (sl - q < 17) return CORRUPT;
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) return CORRUPT;
                Huff& h = tc ? H.ac[th] : H.dc[th];
                int total = 0;
                h.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) total += (h.bits[l] = s[q + l]);
                q += 17;
                if (total > 256 || (size_t)total > sl - q) return CORRUPT;
                memcpy(h.vals, s + q, (size_t)total);
                h.nvals = total;
                q += (size_t)total;
                if (derive(h) != OK) return CORRUPT;
                h.defined = true;
            }
        } else if (m == 0xDB) {
            size_t q = 0;
            while (q < sl) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                if (pq > 1 || tq > 3) return CORRUPT;
                const size_t need = pq ? 128 : 64;
                ++q;
                if (sl - q < need) return CORRUPT;
                for (int i = 0; i < 64; ++i) H.qt[tq][ZIGZAG[i]] = pq ? (uint16_t)be16(s + q + 2 * i) : (uint16_t)s[q + i];
                H.qt_defined[tq] = true;
                q += need;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return CORRUPT;
            H.restart = (int)be16(s);
        } else if (m == 0xE0) {
            if (sl >= 14 && s[0] == 'J' && s[1] == 'F' && s[2] == 'I' && s[3] == 'F' && s[4] == 0) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && s[0] == 'A' && s[1] == 'd' && s[2] == 'o' && s[3] == 'b' && s[4] == 'e') {
                adobe = true;
                adobe_transform = s[11];
            }
        } else if (m == 0xDA) {
            if (!sof) return CORRUPT;
            if (sl < 1) return CORRUPT;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl != (size_t)4 + 2 * (size_t)ns) return CORRUPT;
            if (ns != H.ncomp) return UNSUPPORTED;                             // several scans
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != H.comp[c].id) return UNSUPPORTED;         // components in another order
                H.comp[c].td = s[2 + 2 * c] >> 4;
                H.comp[c].ta = s[2 + 2 * c] & 15;
                if (H.comp[c].td > 3 || H.comp[c].ta > 3) return CORRUPT;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return UNSUPPORTED;
            H.scan = p + len;
            break;
        }
        p += len;
    }
    // the forms the device path rebuilds
    if (H.ncomp == 1) {
        if (H.comp[0].h != 1 || H.comp[0].v != 1) return UNSUPPORTED;
    } else {
        const Component* k = H.comp;
        const bool ycc = jfif ? true : adobe ? adobe_transform == 1 : !(k[0].id == 'R' && k[1].id == 'G' && k[2].id == 'B');
        if (!ycc) return UNSUPPORTED;
        if (k[1].h != 1 || k[1].v != 1 || k[2].h != 1 || k[2].v != 1) return UNSUPPORTED;
        if (!((k[0].h == 1 && k[0].v == 1) || (k[0].h == 2 && k[0].v == 1) || (k[0].h == 2 && k[0].v == 2))) return UNSUPPORTED;
    }
    H.hmax = H.comp[0].h;
    H.vmax = H.comp[0].v;
    H.mcus_w = (H.width + 8 * H.hmax - 1) / (8 * H.hmax);
    H.mcus_h = (H.height + 8 * H.vmax - 1) / (8 * H.vmax);
    for (int c = 0; c < H.ncomp; ++c) {
        // a missing table is left to the other decoder to report
        if (!H.qt_defined[H.comp[c].tq] || !H.dc[H.comp[c].td].defined || !H.ac[H.comp[c].ta].defined) return UNSUPPORTED;
        // libjpeg keeps its multipliers in 16-bit signed words
        for (int i = 0; i < 64; ++i)
            if (H.qt[H.comp[c].tq][i] > 32767) return UNSUPPORTED;
    }
    // every block takes at least two bits (a DC code and an end-of-block code): a scan shorter than that ends early, and
    // no caller sizes a buffer for an image its bytes cannot hold
    uint64_t blocks = 0;
    for (int c = 0; c < H.ncomp; ++c) blocks += (uint64_t)H.mcus_w * H.comp[c].h * H.mcus_h * H.comp[c].v;
    if (blocks * 2 > (uint64_t)(n - H.scan) * 8) return CORRUPT;
    return OK;
}

inline void fill_info(const Header& H, int64_t* info) {
    for (int i = 0; i < INFO_LEN; ++i) info[i] = 0;
    info[0] = H.width;
    info[1] = H.height;
    info[2] = H.ncomp;
    info[3] = H.hmax;
    info[4] = H.vmax;
    info[6] = H.restart;
    info[7] = H.mcus_w;
    info[8] = H.mcus_h;
    int64_t at = 0;
    for (int c = 0; c < H.ncomp; ++c) {
        const int64_t bw = (int64_t)H.mcus_w * H.comp[c].h, bh = (int64_t)H.mcus_h * H.comp[c].v;
        info[9 + 4 * c] = H.comp[c].h;
        info[10 + 4 * c] = H.comp[c].v;
        info[11 + 4 * c] = bw;
        info[12 + 4 * c] = bh;
        info[21 + c] = at;
        at += bw * bh * 64;
    }
    info[5] = at;
}

inline int probe(const uint8_t* b, size_t n, int64_t* info) {
    Header H;
    const int rc = parse_header(b, n, H);
    if (rc == OK) {
        fill_info(H, info);
    } else {
        for (int i = 0; i < INFO_LEN; ++i) info[i] = 0;
    }
    return rc;
}

// MSB-first bit reader over the entropy-coded segment: removes the 0x00 stuffed behind a 0xFF and stops at a marker or at the end of
// the input.  Past that point it supplies zero bits and counts them (`fake`), so that a look-ahead may peek beyond the data; whoever
// CONSUMES one of them has run past the scan (overrun()).
struct Reader {
    const uint8_t* b;
    size_t n, p;
    uint64_t acc;       // the next bits, left-aligned at bit 63
    int bits, fake;     // bits in acc, of which the last `fake` are not data
    bool stopped;       // at a marker (b[p] == 0xFF, b[p + 1] != 0) or at the end of the input

    void start(const uint8_t* bytes, size_t size, size_t at) {
        b = bytes; n = size; p = at; acc = 0; bits = 0; fake = 0; stopped = false;
    }
    void fill() {
        while (bits <= 56) {
            unsigned v = 0;
            if (!stopped) {
                if (p >= n) {
                    stopped = true;
                } else if (b[p] != 0xFF) {
                    v = b[p++];
                } else if (p + 1 < n && b[p + 1] == 0x00) {
                    v = 0xFF;
                    p += 2;
                } else {
                    stopped = true;        // a marker, or a lone 0xFF as the last byte
                }
            }
            if (stopped) fake += 8;
            acc |= (uint64_t)v << (56 - bits);
            bits += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)(acc >> (64 - k)); }     // 1 <= k <= 32, k <= bits
    void skip(int k) { acc <<= k; bits -= k; }
    bool overrun() const { return bits < fake; }
};

// one Huffman symbol; -1 for a code no length matches.  The caller keeps at least 32 bits in the reader
inline int decode_symbol(Reader& r, const Huff& h) {
    const unsigned e = h.look[r.peek(9)];
    if (e) {
        r.skip((int)(e >> 8));
        return (int)(e & 255);
    }
    const unsigned c16 = r.peek(16);
    for (int l = 10; l <= 16; ++l) {
        const int32_t code = (int32_t)(c16 >> (16 - l));
        if (code <= h.maxcode[l]) {
            const int idx = code + h.valoff[l];
            if (idx < 0 || idx >= h.nvals) return -1;
            r.skip(l);
            return h.vals[idx];
        }
    }
    return -1;
}

// the s-bit magnitude field behind a symbol, sign-extended as the standard's EXTEND does; 1 <= s <= 15
inline int32_t receive_extend(Reader& r, int s) {
    const int32_t v = (int32_t)r.peek(s);
    r.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// -> OK, UNSUPPORTED or CORRUPT.  coef: `capacity` int16 values, written only for OK and only below info[5]; qt: 3 x 64 uint16,
// the table of component c at qt + 64 c in natural order (zero for the components a grey image does not have)
inline int entropy_decode(const uint8_t* b, size_t n, int16_t* coef, size_t capacity, uint16_t* qt) {
    Header H;
    const int rc = parse_header(b, n, H);
    if (rc != OK) return rc;
    int64_t info[INFO_LEN];
    fill_info(H, info);
    if ((uint64_t)info[5] > (uint64_t)capacity) return CORRUPT;          // a buffer sized for another file
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 64; ++i) qt[64 * c + i] = c < H.ncomp ? H.qt[H.comp[c].tq][i] : (uint16_t)0;
    Reader r;
    r.start(b, n, H.scan);
    uint32_t pred[3] = {0, 0, 0};                                         // DC predictors, wrapping like the int libjpeg keeps
    const long mcus = (long)H.mcus_w * H.mcus_h;
    int until_restart = H.restart, next_rst = 0;
    for (long m = 0; m < mcus; ++m) {
        if (H.restart && until_restart == 0) {
            // byte-align (the padding bits are dropped), then exactly the expected RSTn
            r.fill();
            if (!r.stopped || r.overrun()) return CORRUPT;
            size_t q = r.p;
            while (q < n && b[q] == 0xFF) ++q;
            if (q >= n || q == r.p || b[q] != 0xD0 + next_rst) return CORRUPT;
            next_rst = (next_rst + 1) & 7;
            r.start(b, n, q + 1);
            pred[0] = pred[1] = pred[2] = 0;
            until_restart = H.restart;
        }
        --until_restart;
        const long my = m / H.mcus_w, mx = m - my * H.mcus_w;
        for (int c = 0; c < H.ncomp; ++c) {
            const Component& k = H.comp[c];
            const Huff &hd = H.dc[k.td], &ha = H.ac[k.ta];
            const int64_t bw = info[11 + 4 * c];
            for (int by = 0; by < k.v; ++by) {
                for (int bx = 0; bx < k.h; ++bx) {
                    int16_t* blk = coef + info[21 + c] + ((my * k.v + by) * bw + (mx * k.h + bx)) * 64;
                    memset(blk, 0, 64 * sizeof(int16_t));
                    if (r.bits < 32) r.fill();
                    int s = decode_symbol(r, hd);
                    if (s < 0 || s > 15) return CORRUPT;
                    if (s) {
                        if (r.bits < 32) r.fill();
                        pred[c] += (uint32_t)receive_extend(r, s);
                    }
                    blk[0] = (int16_t)(uint16_t)pred[c];
                    for (int i = 1; i < 64; ++i) {
                        if (r.bits < 32) r.fill();
                        const int rs = decode_symbol(r, ha);
                        if (rs < 0) return CORRUPT;
                        const int run = rs >> 4;
                        s = rs & 15;
                        if (s == 0) {
                            if (run != 15) break;                         // end of block
                            if (i + 15 > 63) return CORRUPT;              // sixteen zeros that do not fit
                            i += 15;
                            continue;
                        }
                        i += run;
                        if (i > 63) return CORRUPT;                       // a run past coefficient 63
                        blk[ZIGZAG[i]] = (int16_t)receive_extend(r, s);
                    }
                    if (r.overrun()) return CORRUPT;                      // the scan ended inside this block
                }
            }
        }
    }
    return OK;
}

}  // namespace ga_jpeg
