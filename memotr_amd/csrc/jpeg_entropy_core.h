// jpeg_entropy_core.h -- the host half of the JPEG decoder: marker parsing and Huffman decoding of one baseline /
// extended-sequential 8-bit stream into de-zigzagged int16 coefficient blocks and natural-order quantisation tables.
// Plain C++17, no HIP, no allocation, no global state: libjpeg_ops_hip.so includes it (csrc/jpeg_ops.hip), and so
// do the CPU tests (tests/native/jpeg_entropy_fuzz.cpp, g++ with sanitizers).
//
// Accepted: SOF0 / SOF1 at 8 bits, one interleaved scan, 1 component or 3 components (YCbCr) with luma sampling 1x1,
// 2x1 or 2x2 and chroma 1x1, 8- and 16-bit DQT, DHT redefinitions, DRI / RSTn, 0xFF00 stuffing, APPn / COM skipped,
// fill bytes before markers.  Everything else returns one of the codes below with a message; nothing is read past
// `bytes + n` and nothing is written outside `coef` (coef_bytes) and `qt` (3 * 64), whatever the input holds.
//
// Output ("JPEG decode"): component c's blocks are a dense row-major array of blocks_h[c] x blocks_w[c]
// blocks (whole MCUs: the padding blocks of the stream are kept), each 64 int16 in natural order, at
// coef + coef_offset[c]; every block is written whole, zeros included.
#ifndef MEMOTR_JPEG_ENTROPY_CORE_H
#define MEMOTR_JPEG_ENTROPY_CORE_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace jpegcore {

enum Status : int {
    OK = 0,
    ERR_ARGUMENT = 1,          // null pointer, output buffer too small
    ERR_NOT_JPEG = 2,          // no SOI at the start
    ERR_TRUNCATED = 3,         // the data (or the scan, at a marker) ends before the last MCU
    ERR_BAD_SEGMENT = 4,       // a marker segment's length or content is malformed
    ERR_MISSING_TABLE = 5,     // a scan component names a DQT / DHT that was never defined
    ERR_BAD_HUFFMAN_CODE = 6,  // a code that is not in the table
    ERR_COEF_INDEX = 7,        // a coefficient index past 63
    ERR_BAD_RESTART = 8,       // no RSTn, or the wrong one, where the restart interval ends
    ERR_ZERO_DIMENSION = 9,    // width or height 0
    // unsupported kinds of stream (a complete decoder would read them): >= 16
    ERR_PROGRESSIVE = 16,
    ERR_ARITHMETIC = 17,
    ERR_PRECISION = 18,        // not 8 bits per sample
    ERR_COMPONENTS = 19,       // not 1 or 3 components
    ERR_COLOUR_TRANSFORM = 20, // Adobe transform 0 (RGB) or 2 (YCCK), or components named R, G, B
    ERR_SAMPLING = 21,         // sampling factors other than 4:4:4, 4:2:2 (2x1), 4:2:0 (2x2)
    ERR_MULTIPLE_SCANS = 22,
    ERR_SOF_KIND = 23,         // lossless / hierarchical frames
};

inline bool is_unsupported(int status) { return status >= 16; }

struct Info {                  // (the layout of jpegops_info in include/jpeg_ops_hip.h)
    int32_t width, height, ncomp, hmax, vmax, restart_interval, mcus_x, mcus_y;
    int32_t h[3], v[3], blocks_w[3], blocks_h[3];
    int64_t coef_offset[3];    // in int16 elements
    int64_t coef_count;        // int16 elements of all components
};

constexpr int ERR_LEN = 256;

namespace detail {

constexpr uint8_t NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int LOOK_BITS = 9;

struct HuffTable {
    bool defined;
    uint16_t look[1 << LOOK_BITS];     // (length << 8) | symbol for codes of up to LOOK_BITS bits, 0: a longer code
    int32_t maxcode[18];               // largest code of each length, -1: none
    int32_t valoffset[17];             // vals index of the first code of a length, minus that code
    uint8_t vals[256];
};

struct Component {
    int id, h, v, tq, td, ta;
};

struct Parser {
    const uint8_t *p, *end;
    Info info;
    Component comp[3];
    bool have_sof, have_qt[4], jfif, adobe;
    int adobe_transform;
    uint16_t qt[4][64];                // natural order
    HuffTable dc[4], ac[4];
    char *err;

    int fail(int code, const char *msg) {
        if (err) snprintf(err, ERR_LEN, "%s", msg);
        return code;
    }
};

inline int build_table(Parser &s, HuffTable &t, const uint8_t *counts, const uint8_t *vals, int nvals, bool is_dc) {
    uint8_t size[257];
    uint32_t code_of[257];
    int n = 0;
    for (int l = 1; l <= 16; ++l)
        for (int i = 0; i < counts[l - 1]; ++i) size[n++] = (uint8_t)l;
    if (n != nvals || n > 256) return s.fail(ERR_BAD_SEGMENT, "DHT: code counts do not match the segment");
    size[n] = 0;
    uint32_t code = 0;
    int si = n ? size[0] : 0, k = 0;
    while (k < n) {
        while (k < n && size[k] == si) code_of[k++] = code++;
        if (code > (1u << si)) return s.fail(ERR_BAD_SEGMENT, "DHT: more codes of a length than the length holds");
        code <<= 1;
        ++si;
    }
    memset(t.look, 0, sizeof(t.look));
    k = 0;
    for (int l = 1; l <= 16; ++l) {
        if (counts[l - 1]) {
            t.valoffset[l] = k - (int32_t)code_of[k];
            k += counts[l - 1];
            t.maxcode[l] = (int32_t)code_of[k - 1];
        } else {
            t.valoffset[l] = 0;
            t.maxcode[l] = -1;
        }
    }
    t.maxcode[17] = 0x7fffffff;
    for (int i = 0; i < n; ++i) {
        if (is_dc && vals[i] > 15) return s.fail(ERR_BAD_SEGMENT, "DHT: a DC symbol above 15");
        t.vals[i] = vals[i];
        if (size[i] <= LOOK_BITS) {
            const int shift = LOOK_BITS - size[i];
            const uint32_t first = code_of[i] << shift;
            for (uint32_t j = 0; j < (1u << shift); ++j) t.look[first + j] = (uint16_t)((size[i] << 8) | vals[i]);
        }
    }
    for (int i = n; i < 256; ++i) t.vals[i] = 0;
    t.defined = true;
    return OK;
}

inline int read_dqt(Parser &s, const uint8_t *seg, int len) {
    int i = 0;
    while (i < len) {
        const int pq = seg[i] >> 4, tq = seg[i] & 15;
        ++i;
        if (pq > 1 || tq > 3) return s.fail(ERR_BAD_SEGMENT, "DQT: bad precision or table number");
        const int need = pq ? 128 : 64;
        if (len - i < need) return s.fail(ERR_BAD_SEGMENT, "DQT: the segment is shorter than its table");
        for (int k = 0; k < 64; ++k) {
            const int q = pq ? (seg[i + 2 * k] << 8) | seg[i + 2 * k + 1] : seg[i + k];
            s.qt[tq][NATURAL[k]] = (uint16_t)q;
        }
        i += need;
        s.have_qt[tq] = true;
    }
    return OK;
}

inline int read_dht(Parser &s, const uint8_t *seg, int len) {
    int i = 0;
    while (i < len) {
        if (len - i < 17) return s.fail(ERR_BAD_SEGMENT, "DHT: the segment is shorter than its code counts");
        const int tc = seg[i] >> 4, th = seg[i] & 15;
        if (tc > 1 || th > 3) return s.fail(ERR_BAD_SEGMENT, "DHT: bad class or table number");
        const uint8_t *counts = seg + i + 1;
        int n = 0;
        for (int l = 0; l < 16; ++l) n += counts[l];
        i += 17;
        if (n > 256 || len - i < n) return s.fail(ERR_BAD_SEGMENT, "DHT: the segment is shorter than its symbols");
        const int rc = build_table(s, tc ? s.ac[th] : s.dc[th], counts, seg + i, n, tc == 0);
        if (rc) return rc;
        i += n;
    }
    return OK;
}

inline int read_sof(Parser &s, int marker, const uint8_t *seg, int len) {
    if (marker == 0xC2) return s.fail(ERR_PROGRESSIVE, "progressive JPEG (SOF2) is not supported");
    if (marker >= 0xC9) return s.fail(ERR_ARITHMETIC, "arithmetic-coded JPEG is not supported");
    if (marker != 0xC0 && marker != 0xC1) return s.fail(ERR_SOF_KIND, "lossless or hierarchical JPEG is not supported");
    if (s.have_sof) return s.fail(ERR_BAD_SEGMENT, "a second SOF segment");
    if (len < 6) return s.fail(ERR_BAD_SEGMENT, "SOF: the segment is too short");
    if (seg[0] != 8) return s.fail(ERR_PRECISION, "only 8-bit precision is supported");
    Info &f = s.info;
    f.height = (seg[1] << 8) | seg[2];
    f.width = (seg[3] << 8) | seg[4];
    f.ncomp = seg[5];
    if (f.ncomp != 1 && f.ncomp != 3) return s.fail(ERR_COMPONENTS, "only 1 or 3 components are supported");
    if (len != 6 + 3 * f.ncomp) return s.fail(ERR_BAD_SEGMENT, "SOF: the length does not match the component count");
    if (f.width == 0 || f.height == 0) return s.fail(ERR_ZERO_DIMENSION, "width or height is 0");
    for (int c = 0; c < f.ncomp; ++c) {
        Component &k = s.comp[c];
        k.id = seg[6 + 3 * c];
        k.h = seg[7 + 3 * c] >> 4;
        k.v = seg[7 + 3 * c] & 15;
        k.tq = seg[8 + 3 * c];
        if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4 || k.tq > 3)
            return s.fail(ERR_BAD_SEGMENT, "SOF: bad sampling factor or table number");
    }
    if (f.ncomp == 1) {
        s.comp[0].h = s.comp[0].v = 1;         // one component is never interleaved: its factors mean nothing
    } else {
        const int h0 = s.comp[0].h, v0 = s.comp[0].v;
        const bool chroma_ok = s.comp[1].h == 1 && s.comp[1].v == 1 && s.comp[2].h == 1 && s.comp[2].v == 1;
        const bool luma_ok = (h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2);
        if (!chroma_ok || !luma_ok)
            return s.fail(ERR_SAMPLING, "only 4:4:4, 4:2:2 (2x1) and 4:2:0 (2x2) sampling are supported");
    }
    f.hmax = s.comp[0].h;
    f.vmax = s.comp[0].v;
    f.mcus_x = (f.width + 8 * f.hmax - 1) / (8 * f.hmax);
    f.mcus_y = (f.height + 8 * f.vmax - 1) / (8 * f.vmax);
    int64_t off = 0;
    for (int c = 0; c < 3; ++c) {
        const bool live = c < f.ncomp;
        f.h[c] = live ? s.comp[c].h : 0;
        f.v[c] = live ? s.comp[c].v : 0;
        f.blocks_w[c] = live ? f.mcus_x * s.comp[c].h : 0;
        f.blocks_h[c] = live ? f.mcus_y * s.comp[c].v : 0;
        f.coef_offset[c] = off;
        off += (int64_t)f.blocks_w[c] * f.blocks_h[c] * 64;
    }
    f.coef_count = off;
    s.have_sof = true;
    return OK;
}

inline int colour_check(Parser &s) {
    if (s.info.ncomp != 3) return OK;
    if (s.adobe) {
        if (s.adobe_transform != 1)
            return s.fail(ERR_COLOUR_TRANSFORM, s.adobe_transform == 2
                                                    ? "Adobe transform 2 (YCCK) is not supported"
                                                    : "Adobe transform 0 (RGB, no colour transform) is not supported");
    } else if (!s.jfif && s.comp[0].id == 'R' && s.comp[1].id == 'G' && s.comp[2].id == 'B') {
        return s.fail(ERR_COLOUR_TRANSFORM, "components named R, G, B (no colour transform) are not supported");
    }
    return OK;
}

// Walks the marker segments up to and including SOS.  On OK, s.p is the first byte of entropy-coded data.
inline int read_headers(Parser &s) {
    if (s.end - s.p < 2 || s.p[0] != 0xFF || s.p[1] != 0xD8) return s.fail(ERR_NOT_JPEG, "not a JPEG stream (no SOI)");
    s.p += 2;
    for (;;) {
        // a marker: 0xFF, any number of 0xFF fill bytes, the code
        if (s.p >= s.end) return s.fail(ERR_TRUNCATED, "the data ends before the scan");
        if (*s.p != 0xFF) return s.fail(ERR_BAD_SEGMENT, "a marker was expected");
        while (s.p < s.end && *s.p == 0xFF) ++s.p;
        if (s.p >= s.end) return s.fail(ERR_TRUNCATED, "the data ends before the scan");
        const int m = *s.p++;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;       // no payload
        if (m == 0xD9) return s.fail(ERR_TRUNCATED, "EOI before the scan");
        if (m == 0x00) return s.fail(ERR_BAD_SEGMENT, "a marker was expected");
        if (s.end - s.p < 2) return s.fail(ERR_TRUNCATED, "the data ends inside a marker segment");
        const int len = ((s.p[0] << 8) | s.p[1]) - 2;
        if (len < 0) return s.fail(ERR_BAD_SEGMENT, "a segment length below 2");
        if (s.end - s.p - 2 < len) return s.fail(ERR_TRUNCATED, "the data ends inside a marker segment");
        const uint8_t *seg = s.p + 2;
        s.p = seg + len;
        int rc = OK;
        if (m == 0xDB) {
            rc = read_dqt(s, seg, len);
        } else if (m == 0xC4) {
            rc = read_dht(s, seg, len);
        } else if (m == 0xCC) {
            rc = s.fail(ERR_ARITHMETIC, "arithmetic-coded JPEG is not supported");
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8) {
            rc = read_sof(s, m, seg, len);
            if (rc == OK) rc = colour_check(s);
        } else if (m == 0xDD) {
            if (len != 2) return s.fail(ERR_BAD_SEGMENT, "DRI: bad length");
            s.info.restart_interval = (seg[0] << 8) | seg[1];
        } else if (m == 0xE0) {
            if (len >= 5 && memcmp(seg, "JFIF", 5) == 0) s.jfif = true;
        } else if (m == 0xEE) {
            if (len >= 12 && memcmp(seg, "Adobe", 5) == 0) {
                s.adobe = true;
                s.adobe_transform = seg[11];
                if (s.have_sof) rc = colour_check(s);
            }
        } else if (m == 0xDA) {
            if (!s.have_sof) return s.fail(ERR_BAD_SEGMENT, "SOS before SOF");
            if (len < 1) return s.fail(ERR_BAD_SEGMENT, "SOS: the segment is too short");
            const int ns = seg[0];
            if (ns < 1 || ns > 4) return s.fail(ERR_BAD_SEGMENT, "SOS: bad component count");
            if (ns != s.info.ncomp)
                return s.fail(ERR_MULTIPLE_SCANS, "a scan without all components (multiple scans) is not supported");
            if (len != 4 + 2 * ns) return s.fail(ERR_BAD_SEGMENT, "SOS: bad length");
            for (int c = 0; c < ns; ++c) {
                if (seg[1 + 2 * c] != s.comp[c].id)
                    return s.fail(ERR_BAD_SEGMENT, "SOS: component order differs from SOF");
                s.comp[c].td = seg[2 + 2 * c] >> 4;
                s.comp[c].ta = seg[2 + 2 * c] & 15;
                if (s.comp[c].td > 3 || s.comp[c].ta > 3) return s.fail(ERR_BAD_SEGMENT, "SOS: bad table number");
                if (!s.dc[s.comp[c].td].defined || !s.ac[s.comp[c].ta].defined)
                    return s.fail(ERR_MISSING_TABLE, "the scan names a Huffman table that is not defined");
                if (!s.have_qt[s.comp[c].tq])
                    return s.fail(ERR_MISSING_TABLE, "a component names a quantisation table that is not defined");
            }
            const uint8_t *t = seg + 1 + 2 * ns;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0)
                return s.fail(ERR_BAD_SEGMENT, "SOS: spectral selection of a sequential scan is not 0..63");
            return OK;
        }
        // everything else (APPn, COM, DNL, ...) is skipped
        if (rc) return rc;
    }
}

// MSB-first bit reader over entropy-coded data.  It never advances past a marker or `end`; from there on it
// supplies zero bits and counts them (`fake`): a decoder that consumed one of those has run out of data.
struct BitReader {
    const uint8_t *p, *end;
    uint64_t acc;
    int bits, fake;
    bool stopped;

    inline void fill() {
        if (!stopped && bits <= 32 && end - p >= 4) {      // four bytes at once when none of them is 0xFF
            uint32_t v;
            memcpy(&v, p, 4);
            if (((~v - 0x01010101u) & v & 0x80808080u) == 0) {
                acc = (acc << 32) | __builtin_bswap32(v);
                bits += 32;
                p += 4;
            }
        }
        while (bits <= 56) {
            uint32_t b = 0;
            if (!stopped) {
                if (p < end && *p != 0xFF) {
                    b = *p++;
                } else if (end - p >= 2 && p[1] == 0x00) {
                    b = 0xFF;
                    p += 2;
                } else {
                    stopped = true;
                }
            }
            if (stopped) fake += 8;
            acc = (acc << 8) | b;
            bits += 8;
        }
    }
    inline uint32_t peek(int n) const { return (uint32_t)(acc >> (bits - n)) & ((1u << n) - 1u); }
    inline bool overrun() const { return bits < fake; }
};

inline int decode_symbol(BitReader &br, const HuffTable &t) {
    if (br.bits < 32) br.fill();
    const uint16_t e = t.look[br.peek(LOOK_BITS)];
    if (e) {
        br.bits -= e >> 8;
        return e & 255;
    }
    int l = LOOK_BITS + 1;
    int32_t code = (int32_t)br.peek(l);
    while (l <= 16 && code > t.maxcode[l]) {
        ++l;
        if (l <= 16) code = (int32_t)br.peek(l);
    }
    if (l > 16) return -1;
    br.bits -= l;
    return t.vals[(code + t.valoffset[l]) & 255];
}

inline int receive_extend(BitReader &br, int s) {        // s in 1..15, at least s bits are in the accumulator
    const int v = (int)br.peek(s);
    br.bits -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

inline int decode_block(Parser &s, BitReader &br, const HuffTable &dc, const HuffTable &ac, int &pred, int16_t *blk) {
    memset(blk, 0, 64 * sizeof(int16_t));
    int sym = decode_symbol(br, dc);
    if (sym < 0) return s.fail(ERR_BAD_HUFFMAN_CODE, "a Huffman code that is not in the DC table");
    if (sym) pred += receive_extend(br, sym);
    pred = (int)(int16_t)(uint16_t)(uint32_t)pred;       // 8-bit streams stay far inside; hostile ones wrap, defined
    blk[0] = (int16_t)pred;
    for (int k = 1; k < 64; ++k) {
        sym = decode_symbol(br, ac);
        if (sym < 0) return s.fail(ERR_BAD_HUFFMAN_CODE, "a Huffman code that is not in the AC table");
        const int r = sym >> 4, n = sym & 15;
        if (n) {
            k += r;
            if (k > 63) return s.fail(ERR_COEF_INDEX, "a coefficient index past 63");
            blk[NATURAL[k]] = (int16_t)receive_extend(br, n);
        } else if (r == 15) {
            k += 15;
        } else {
            break;
        }
    }
    return OK;
}

inline void init(Parser &s, const uint8_t *bytes, size_t n, char *err) {
    memset(&s, 0, sizeof(s));
    s.p = bytes;
    s.end = bytes + n;
    s.err = err;
    if (err) err[0] = 0;
}

}  // namespace detail

// Sizes only (the marker segments up to the scan, no entropy-coded data): what the caller needs to allocate.
inline int parse_header(const uint8_t *bytes, size_t n, Info *info, char *err) {
    if (err) err[0] = 0;
    if (!bytes || !info) {
        if (err) snprintf(err, ERR_LEN, "null pointer");
        return ERR_ARGUMENT;
    }
    detail::Parser s;
    detail::init(s, bytes, n, err);
    const int rc = detail::read_headers(s);
    if (rc == OK) *info = s.info;
    return rc;
}

// The whole host stage.  coef: at least info->coef_count int16 (coef_bytes is checked); qt: 3 * 64 uint16, rows of
// components the stream does not have are zeroed.  *info is written on success.
inline int decode(const uint8_t *bytes, size_t n, Info *info, int16_t *coef, size_t coef_bytes, uint16_t *qt, char *err) {
    using namespace detail;
    if (err) err[0] = 0;
    if (!bytes || !info || !coef || !qt) {
        if (err) snprintf(err, ERR_LEN, "null pointer");
        return ERR_ARGUMENT;
    }
    Parser s;
    init(s, bytes, n, err);
    int rc = read_headers(s);
    if (rc) return rc;
    const Info &f = s.info;
    if ((uint64_t)f.coef_count * sizeof(int16_t) > (uint64_t)coef_bytes)
        return s.fail(ERR_ARGUMENT, "the coefficient buffer is smaller than the image needs");
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 64; ++k) qt[c * 64 + k] = c < f.ncomp ? s.qt[s.comp[c].tq][k] : 0;

    BitReader br = {s.p, s.end, 0, 0, 0, false};
    int pred[3] = {0, 0, 0};
    const int interval = f.restart_interval;
    int left = interval, next_rst = 0;
    for (int my = 0; my < f.mcus_y; ++my) {
        for (int mx = 0; mx < f.mcus_x; ++mx) {
            if (interval && left == 0) {
                // byte-align, then RSTn (after fill bytes); less than one byte of padding may be left over
                if (!br.stopped) br.fill();
                if (!br.stopped || br.bits - br.fake >= 8)      // whole bytes of data where the marker belongs
                    return s.fail(ERR_BAD_RESTART, "no restart marker where the restart interval ends");
                const uint8_t *q = br.p;
                while (q < s.end && *q == 0xFF) ++q;
                if (q >= s.end || q == br.p) return s.fail(ERR_TRUNCATED, "the data ends before the last MCU");
                if (*q >= 0xD0 && *q <= 0xD7 && *q != 0xD0 + next_rst)
                    return s.fail(ERR_BAD_RESTART, "restart markers out of order");
                if (*q != 0xD0 + next_rst) return s.fail(ERR_TRUNCATED, "the scan ends before the last MCU");
                br = {q + 1, s.end, 0, 0, 0, false};
                next_rst = (next_rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
                left = interval;
            }
            for (int c = 0; c < f.ncomp; ++c) {
                const HuffTable &dc = s.dc[s.comp[c].td], &ac = s.ac[s.comp[c].ta];
                for (int by = 0; by < f.v[c]; ++by) {
                    for (int bx = 0; bx < f.h[c]; ++bx) {
                        const int64_t row = (int64_t)my * f.v[c] + by, col = (int64_t)mx * f.h[c] + bx;
                        int16_t *blk = coef + f.coef_offset[c] + (row * f.blocks_w[c] + col) * 64;
                        rc = decode_block(s, br, dc, ac, pred[c], blk);
                        if (rc) return rc;
                    }
                }
            }
            if (br.overrun()) return s.fail(ERR_TRUNCATED, "the data ends before the last MCU");
            --left;
        }
    }
    *info = f;
    return OK;
}

}  // namespace jpegcore

#endif  // MEMOTR_JPEG_ENTROPY_CORE_H
