// jpeg_encode_core.h -- the host stage of the baseline JPEG encoder: quantisation tables, the marker segments and
// the Huffman-coded scan, from int16 coefficient blocks to the bytes of a file.  Plain C++17: no HIP, no allocation,
// no global state; compiled into libjpeg_enc_hip.so (jpeg_enc.hip) and into a stand-alone sanitizer program
// (tests/native/jpeg_encode_check.cpp).
//
// Scope: 8-bit, three components, 4:4:4 (hmax = vmax = 1) or 4:2:0 (hmax = vmax = 2), quality 1 .. 100, the Annex K
// tables unoptimised, no restart markers.  The bytes are the ones libjpeg-turbo (Pillow's Image.save) writes for the
// same coefficients:
//
//   SOI, APP0 (JFIF 1.01, units 0, density 1 x 1, no thumbnail), DQT luma, DQT chroma (8-bit entries, zigzag order),
//   SOF0 (component ids 1, 2, 3; sampling 0x22 / 0x11 / 0x11 or all 0x11; tables 0, 1, 1), DHT DC0, AC0, DC1, AC1 (a
//   segment each), SOS, the MCU-interleaved scan (DC differences per component, AC run / size with ZRL and EOB, a zero
//   byte stuffed after every 0xFF, the last byte padded with one-bits), EOI.
//
// The writer never stores past the caller's buffer: it counts every byte and stores the ones that fit, so the return
// value is the size the stream needs whether or not it fitted.
#ifndef JPEG_ENCODE_CORE_H
#define JPEG_ENCODE_CORE_H

#include <stddef.h>
#include <stdint.h>

namespace jpegenc {

// Block geometry of a frame: the layout of jpegcore::Info (jpeg_entropy_core.h) and of jpegenc_info (the C ABI).
struct Info {
    int32_t width, height, ncomp, hmax, vmax, restart_interval, mcus_x, mcus_y;
    int32_t h[3], v[3], blocks_w[3], blocks_h[3];
    int64_t coef_offset[3];
    int64_t coef_count;
};

constexpr int ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.1 and K.2, in zigzag order (what a quality-50 stream's DQT segments hold).
constexpr uint8_t BASE_QT[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13,  14,  18, 17, 16, 19, 24,  40,  26,  24,  22,  22,  24, 49,
     35, 37, 29, 40, 58, 51, 61, 60, 57,  51,  56, 55, 64, 72, 92,  78,  64,  68,  87,  69,  55, 56,
     80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3 - K.6: code counts per length 1 .. 16, then the symbols.  Index: 0 DC luma, 1 AC luma, 2 DC chroma,
// 3 AC chroma (the order of the DHT segments).
constexpr uint8_t HUFF_BITS[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                      {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                      {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                      {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr int HUFF_COUNT[4] = {12, 162, 12, 162};
constexpr uint8_t HUFF_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t HUFF_AC_LUMA_VALS[162] = {
    1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161,
    8,   35,  66,  177, 193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,
    39,  40,  41,  42,  52,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,
    87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133,
    134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
    178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214,
    215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249,
    250};
constexpr uint8_t HUFF_AC_CHROMA_VALS[162] = {
    0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,
    145, 161, 177, 193, 9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,
    26,  38,  39,  40,  41,  42,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,
    86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131,
    132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168,
    169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212,
    213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249,
    250};

inline const uint8_t *huff_vals(int t) {
    return t == 1 ? HUFF_AC_LUMA_VALS : t == 3 ? HUFF_AC_CHROMA_VALS : HUFF_DC_VALS;
}

// libjpeg's quality scaling.  out: uint16[3][64], natural order, component 0 luma, 1 and 2 chroma (the layout the
// decoder's host stage writes).  Returns 0, or 1 for a quality outside 1 .. 100.
inline int quant_tables(int quality, uint16_t *out) {
    if (quality < 1 || quality > 100) return 1;
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 64; ++k) {
            int v = (BASE_QT[c ? 1 : 0][k] * s + 50) / 100;
            v = v < 1 ? 1 : (v > 255 ? 255 : v);
            out[c * 64 + ZIGZAG[k]] = (uint16_t)v;
        }
    return 0;
}

// Whole-MCU geometry of a width x height frame with luma sampling hmax x hmax (1: 4:4:4, 2: 4:2:0).
// Returns 0, or 1 for a size outside 1 .. 65535 or another sampling.
inline int geometry(int width, int height, int hmax, Info *f) {
    if (width < 1 || height < 1 || width > 65535 || height > 65535 || (hmax != 1 && hmax != 2)) return 1;
    f->width = width; f->height = height; f->ncomp = 3; f->hmax = f->vmax = hmax; f->restart_interval = 0;
    f->mcus_x = (width + 8 * hmax - 1) / (8 * hmax);
    f->mcus_y = (height + 8 * hmax - 1) / (8 * hmax);
    int64_t off = 0;
    for (int c = 0; c < 3; ++c) {
        f->h[c] = f->v[c] = c == 0 ? hmax : 1;
        f->blocks_w[c] = f->mcus_x * f->h[c];
        f->blocks_h[c] = f->mcus_y * f->v[c];
        f->coef_offset[c] = off;
        off += (int64_t)f->blocks_w[c] * f->blocks_h[c] * 64;
    }
    f->coef_count = off;
    return 0;
}

inline bool same_geometry(const Info &a, const Info &b) {
    if (a.width != b.width || a.height != b.height || a.ncomp != b.ncomp || a.hmax != b.hmax || a.vmax != b.vmax ||
        a.restart_interval != b.restart_interval || a.mcus_x != b.mcus_x || a.mcus_y != b.mcus_y ||
        a.coef_count != b.coef_count)
        return false;
    for (int c = 0; c < 3; ++c)
        if (a.h[c] != b.h[c] || a.v[c] != b.v[c] || a.blocks_w[c] != b.blocks_w[c] || a.blocks_h[c] != b.blocks_h[c] ||
            a.coef_offset[c] != b.coef_offset[c])
            return false;
    return true;
}

// 0 when `f` is what geometry() makes for its own width, height and hmax.
inline int check_info(const Info *f) {
    Info want;
    if (f->hmax != f->vmax || geometry(f->width, f->height, f->hmax, &want)) return 1;
    return same_geometry(*f, want) ? 0 : 1;
}

struct HuffTable {
    uint16_t code[256];
    uint8_t size[256];      // 0: the symbol has no code
};

inline void make_table(int t, HuffTable *h) {
    for (int i = 0; i < 256; ++i) { h->code[i] = 0; h->size[i] = 0; }
    const uint8_t *vals = huff_vals(t);
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < HUFF_BITS[t][len - 1]; ++i, ++k) {
            h->code[vals[k]] = (uint16_t)code++;
            h->size[vals[k]] = (uint8_t)len;
        }
        code <<= 1;
    }
}

// Counts every byte, stores the ones below `cap`.
struct Writer {
    uint8_t *out;
    size_t cap, pos;
    uint64_t acc;           // pending bits, right-aligned: fewer than 32 between calls
    int nbits;

    void byte(unsigned b) {
        if (pos < cap) out[pos] = (uint8_t)b;
        ++pos;
    }
    void u16(unsigned v) { byte(v >> 8); byte(v & 255); }
    void scan_byte(unsigned b) {
        byte(b);
        if (b == 255) byte(0);
    }
    void bits(unsigned code, int size) {             // size <= 26, code < 2^size
        acc = (acc << size) | code;
        nbits += size;
        if (nbits < 32) return;
        nbits -= 32;
        const uint32_t w = (uint32_t)(acc >> nbits);
        if (pos + 4 <= cap && ((~w - 0x01010101u) & w & 0x80808080u) == 0) {        // room, and no 0xFF among the four
            out[pos] = (uint8_t)(w >> 24); out[pos + 1] = (uint8_t)(w >> 16); out[pos + 2] = (uint8_t)(w >> 8);
            out[pos + 3] = (uint8_t)w;
            pos += 4;
        } else {
            scan_byte(w >> 24); scan_byte((w >> 16) & 255); scan_byte((w >> 8) & 255); scan_byte(w & 255);
        }
    }
    void flush() {
        while (nbits >= 8) {
            nbits -= 8;
            scan_byte((unsigned)(acc >> nbits) & 255);
        }
        if (nbits > 0) {
            scan_byte((((unsigned)acc << (8 - nbits)) | ((1u << (8 - nbits)) - 1)) & 255);
            nbits = 0;
        }
    }
};

inline int bit_size(unsigned v) {
#if defined(__GNUC__) || defined(__clang__)
    return v ? 32 - __builtin_clz(v) : 0;
#else
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
#endif
}

inline int lowest_bit(uint64_t m) {                  // m != 0
#if defined(__GNUC__) || defined(__clang__)
    return __builtin_ctzll(m);
#else
    int k = 0;
    while (!(m & 1)) { m >>= 1; ++k; }
    return k;
#endif
}

// One block of 64 int16 in natural order.  Values outside what 8-bit baseline coding can express (DC difference of
// more than 11 bits, AC of more than 10) make the stream invalid: returns false.
inline bool encode_block(Writer &w, const int16_t *blk, int *last_dc, const HuffTable &dc, const HuffTable &ac) {
    const int diff = (int)blk[0] - *last_dc;
    *last_dc = blk[0];
    int n = bit_size((unsigned)(diff < 0 ? -diff : diff));
    if (n > 11) return false;
    // the code and the value bits behind it go out as one field (a negative value as its low bits minus one)
    w.bits(((unsigned)dc.code[n] << n) | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1)), dc.size[n] + n);
    // the block in zigzag order and a bit per non-zero coefficient: the loop below visits only those
    int16_t t[64];
    uint64_t mask = 0;
    for (int k = 0; k < 64; ++k) t[k] = blk[ZIGZAG[k]];
    for (int k = 1; k < 64; ++k) mask |= (uint64_t)(t[k] != 0) << k;
    int prev = 0;
    while (mask) {
        const int k = lowest_bit(mask);
        mask &= mask - 1;
        int run = k - prev - 1;
        prev = k;
        while (run > 15) { w.bits(ac.code[0xF0], ac.size[0xF0]); run -= 16; }
        const int v = t[k];
        n = bit_size((unsigned)(v < 0 ? -v : v));
        if (n > 10) return false;
        const int sym = (run << 4) | n;
        w.bits(((unsigned)ac.code[sym] << n) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1)), ac.size[sym] + n);
    }
    if (prev != 63) w.bits(ac.code[0], ac.size[0]);
    return true;
}

inline void write_header(Writer &w, const Info &f, const uint16_t *qt) {
    w.u16(0xFFD8);
    w.u16(0xFFE0); w.u16(16);
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (uint8_t b : jfif) w.byte(b);
    for (int t = 0; t < 2; ++t) {
        w.u16(0xFFDB); w.u16(67); w.byte(t);
        for (int k = 0; k < 64; ++k) w.byte(qt[t * 64 + ZIGZAG[k]] & 255);
    }
    w.u16(0xFFC0); w.u16(17); w.byte(8); w.u16(f.height); w.u16(f.width); w.byte(3);
    for (int c = 0; c < 3; ++c) { w.byte(c + 1); w.byte(f.h[c] << 4 | f.v[c]); w.byte(c ? 1 : 0); }
    const int ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) {
        w.u16(0xFFC4); w.u16(19 + HUFF_COUNT[t]); w.byte(ids[t]);
        for (int i = 0; i < 16; ++i) w.byte(HUFF_BITS[t][i]);
        const uint8_t *vals = huff_vals(t);
        for (int i = 0; i < HUFF_COUNT[t]; ++i) w.byte(vals[i]);
    }
    w.u16(0xFFDA); w.u16(12); w.byte(3);
    for (int c = 0; c < 3; ++c) { w.byte(c + 1); w.byte(c ? 0x11 : 0x00); }
    w.byte(0); w.byte(63); w.byte(0);
}

// coef: the frame's coef_count int16 (component c at coef_offset[c], blocks row-major, natural order, dummy blocks
// filled); qt: uint16[3][64] natural order, entries 1 .. 255.  Returns the stream's size in bytes; the stream is in
// out[0 .. size) when size <= cap, and only out[0 .. cap) was touched otherwise.  Returns -1 for a geometry
// geometry() does not make, -2 for a table entry outside 1 .. 255, -3 for a coefficient baseline coding cannot
// express.
inline int64_t encode(const int16_t *coef, const uint16_t *qt, const Info *info, uint8_t *out, size_t cap) {
    if (check_info(info)) return -1;
    for (int k = 0; k < 128; ++k)
        if (qt[k] < 1 || qt[k] > 255) return -2;
    const Info &f = *info;
    Writer w{out, out ? cap : 0, 0, 0, 0};
    write_header(w, f, qt);
    HuffTable tab[4];
    for (int t = 0; t < 4; ++t) make_table(t, &tab[t]);
    int last_dc[3] = {0, 0, 0};
    for (int my = 0; my < f.mcus_y; ++my)
        for (int mx = 0; mx < f.mcus_x; ++mx)
            for (int c = 0; c < 3; ++c)
                for (int v = 0; v < f.v[c]; ++v)
                    for (int h = 0; h < f.h[c]; ++h) {
                        const int64_t b = (int64_t)(my * f.v[c] + v) * f.blocks_w[c] + mx * f.h[c] + h;
                        if (!encode_block(w, coef + f.coef_offset[c] + b * 64, &last_dc[c], tab[c ? 2 : 0],
                                          tab[c ? 3 : 1]))
                            return -3;
                    }
    w.flush();
    w.u16(0xFFD9);
    return (int64_t)w.pos;
}

}  // namespace jpegenc

#endif  // JPEG_ENCODE_CORE_H
