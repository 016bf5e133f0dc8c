// jmcodec_amd/csrc/mpeg2_syntax.cpp -- MPEG-2 video syntax (ISO/IEC 13818-2 6.2, 7.2 - 7.6.3, Annex B): see mpeg2_syntax.h.
#include "mpeg2_syntax.h"
#include <cstdlib>
#include <cstring>

namespace jmamd {

// ---- Annex B ---------------------------------------------------------------------------------------------------------------------------
// B-1 macroblock_address_increment (a = 34: macroblock_escape)
static const Mpeg2Vlc kMba[] = {
    {0x1, 1, 1, 0}, {0x3, 3, 2, 0}, {0x2, 3, 3, 0}, {0x3, 4, 4, 0}, {0x2, 4, 5, 0}, {0x3, 5, 6, 0}, {0x2, 5, 7, 0}, {0x7, 7, 8, 0}, {0x6, 7, 9, 0},
    {0xb, 8, 10, 0}, {0xa, 8, 11, 0}, {0x9, 8, 12, 0}, {0x8, 8, 13, 0}, {0x7, 8, 14, 0}, {0x6, 8, 15, 0}, {0x17, 10, 16, 0}, {0x16, 10, 17, 0},
    {0x15, 10, 18, 0}, {0x14, 10, 19, 0}, {0x13, 10, 20, 0}, {0x12, 10, 21, 0}, {0x23, 11, 22, 0}, {0x22, 11, 23, 0}, {0x21, 11, 24, 0},
    {0x20, 11, 25, 0}, {0x1f, 11, 26, 0}, {0x1e, 11, 27, 0}, {0x1d, 11, 28, 0}, {0x1c, 11, 29, 0}, {0x1b, 11, 30, 0}, {0x1a, 11, 31, 0},
    {0x19, 11, 32, 0}, {0x18, 11, 33, 0}, {0x8, 11, 34, 0}};
// B-2 / B-3 / B-4 macroblock_type: a = quant 1 | forward 2 | backward 4 | pattern 8 | intra 16
static const Mpeg2Vlc kMbTypeI[] = {{0x1, 1, 16, 0}, {0x1, 2, 17, 0}};
static const Mpeg2Vlc kMbTypeP[] = {{0x1, 1, 10, 0}, {0x1, 2, 8, 0}, {0x1, 3, 2, 0}, {0x3, 5, 16, 0}, {0x2, 5, 11, 0}, {0x1, 5, 9, 0}, {0x1, 6, 17, 0}};
static const Mpeg2Vlc kMbTypeB[] = {{0x2, 2, 6, 0}, {0x3, 2, 14, 0}, {0x2, 3, 4, 0}, {0x3, 3, 12, 0}, {0x2, 4, 2, 0}, {0x3, 4, 10, 0}, {0x3, 5, 16, 0},
                                    {0x2, 5, 15, 0}, {0x3, 6, 11, 0}, {0x2, 6, 13, 0}, {0x1, 6, 17, 0}};
// B-9 coded_block_pattern, entry k = cbp k
static const Mpeg2Vlc kCbp[] = {
    {0x1, 9, 0, 0}, {0xb, 5, 1, 0}, {0x9, 5, 2, 0}, {0xd, 6, 3, 0}, {0xd, 4, 4, 0}, {0x17, 7, 5, 0}, {0x13, 7, 6, 0}, {0x1f, 8, 7, 0},
    {0xc, 4, 8, 0}, {0x16, 7, 9, 0}, {0x12, 7, 10, 0}, {0x1e, 8, 11, 0}, {0x13, 5, 12, 0}, {0x1b, 8, 13, 0}, {0x17, 8, 14, 0}, {0x13, 8, 15, 0},
    {0xb, 4, 16, 0}, {0x15, 7, 17, 0}, {0x11, 7, 18, 0}, {0x1d, 8, 19, 0}, {0x11, 5, 20, 0}, {0x19, 8, 21, 0}, {0x15, 8, 22, 0}, {0x11, 8, 23, 0},
    {0xf, 6, 24, 0}, {0xf, 8, 25, 0}, {0xd, 8, 26, 0}, {0x3, 9, 27, 0}, {0xf, 5, 28, 0}, {0xb, 8, 29, 0}, {0x7, 8, 30, 0}, {0x7, 9, 31, 0},
    {0xa, 4, 32, 0}, {0x14, 7, 33, 0}, {0x10, 7, 34, 0}, {0x1c, 8, 35, 0}, {0xe, 6, 36, 0}, {0xe, 8, 37, 0}, {0xc, 8, 38, 0}, {0x2, 9, 39, 0},
    {0x10, 5, 40, 0}, {0x18, 8, 41, 0}, {0x14, 8, 42, 0}, {0x10, 8, 43, 0}, {0xe, 5, 44, 0}, {0xa, 8, 45, 0}, {0x6, 8, 46, 0}, {0x6, 9, 47, 0},
    {0x12, 5, 48, 0}, {0x1a, 8, 49, 0}, {0x16, 8, 50, 0}, {0x12, 8, 51, 0}, {0xd, 5, 52, 0}, {0x9, 8, 53, 0}, {0x5, 8, 54, 0}, {0x5, 9, 55, 0},
    {0xc, 5, 56, 0}, {0x8, 8, 57, 0}, {0x4, 8, 58, 0}, {0x4, 9, 59, 0}, {0x7, 3, 60, 0}, {0xa, 5, 61, 0}, {0x8, 5, 62, 0}, {0xc, 6, 63, 0}};
// B-10 motion_code, magnitudes (codes of a != 0 are followed by the sign bit)
// B-11 dmvector: a = the value
static const Mpeg2Vlc kDmv[] = {{0x0, 1, 0, 0}, {0x2, 2, 1, 0}, {0x3, 2, -1, 0}};
static const Mpeg2Vlc kMotion[] = {{0x1, 1, 0, 0}, {0x1, 2, 1, 0}, {0x1, 3, 2, 0}, {0x1, 4, 3, 0}, {0x3, 6, 4, 0}, {0x5, 7, 5, 0}, {0x4, 7, 6, 0},
                                   {0x3, 7, 7, 0}, {0xb, 9, 8, 0}, {0xa, 9, 9, 0}, {0x9, 9, 10, 0}, {0x11, 10, 11, 0}, {0x10, 10, 12, 0}, {0xf, 10, 13, 0},
                                   {0xe, 10, 14, 0}, {0xd, 10, 15, 0}, {0xc, 10, 16, 0}};
// B-12 / B-13 dct_dc_size_luminance / _chrominance
static const Mpeg2Vlc kDcLuma[] = {{0x4, 3, 0, 0}, {0x0, 2, 1, 0}, {0x1, 2, 2, 0}, {0x5, 3, 3, 0}, {0x6, 3, 4, 0}, {0xe, 4, 5, 0}, {0x1e, 5, 6, 0},
                                   {0x3e, 6, 7, 0}, {0x7e, 7, 8, 0}, {0xfe, 8, 9, 0}, {0x1fe, 9, 10, 0}, {0x1ff, 9, 11, 0}};
static const Mpeg2Vlc kDcChroma[] = {{0x0, 2, 0, 0}, {0x1, 2, 1, 0}, {0x2, 2, 2, 0}, {0x6, 3, 3, 0}, {0xe, 4, 4, 0}, {0x1e, 5, 5, 0}, {0x3e, 6, 6, 0},
                                     {0x7e, 7, 7, 0}, {0xfe, 8, 8, 0}, {0x1fe, 9, 9, 0}, {0x3fe, 10, 10, 0}, {0x3ff, 10, 11, 0}};
// B-14 DCT coefficients table zero: a = run, b = level (the sign bit follows); -1 end of block, -2 escape
static const Mpeg2Vlc kDct0[] = {
    {0x3, 2, 0, 1}, {0x4, 4, 0, 2}, {0x5, 5, 0, 3}, {0x6, 7, 0, 4}, {0x26, 8, 0, 5}, {0x21, 8, 0, 6}, {0xa, 10, 0, 7}, {0x1d, 12, 0, 8},
    {0x18, 12, 0, 9}, {0x13, 12, 0, 10}, {0x10, 12, 0, 11}, {0x1a, 13, 0, 12}, {0x19, 13, 0, 13}, {0x18, 13, 0, 14}, {0x17, 13, 0, 15},
    {0x1f, 14, 0, 16}, {0x1e, 14, 0, 17}, {0x1d, 14, 0, 18}, {0x1c, 14, 0, 19}, {0x1b, 14, 0, 20}, {0x1a, 14, 0, 21}, {0x19, 14, 0, 22},
    {0x18, 14, 0, 23}, {0x17, 14, 0, 24}, {0x16, 14, 0, 25}, {0x15, 14, 0, 26}, {0x14, 14, 0, 27}, {0x13, 14, 0, 28}, {0x12, 14, 0, 29},
    {0x11, 14, 0, 30}, {0x10, 14, 0, 31}, {0x18, 15, 0, 32}, {0x17, 15, 0, 33}, {0x16, 15, 0, 34}, {0x15, 15, 0, 35}, {0x14, 15, 0, 36},
    {0x13, 15, 0, 37}, {0x12, 15, 0, 38}, {0x11, 15, 0, 39}, {0x10, 15, 0, 40},
    {0x3, 3, 1, 1}, {0x6, 6, 1, 2}, {0x25, 8, 1, 3}, {0xc, 10, 1, 4}, {0x1b, 12, 1, 5}, {0x16, 13, 1, 6}, {0x15, 13, 1, 7}, {0x1f, 15, 1, 8},
    {0x1e, 15, 1, 9}, {0x1d, 15, 1, 10}, {0x1c, 15, 1, 11}, {0x1b, 15, 1, 12}, {0x1a, 15, 1, 13}, {0x19, 15, 1, 14}, {0x13, 16, 1, 15},
    {0x12, 16, 1, 16}, {0x11, 16, 1, 17}, {0x10, 16, 1, 18},
    {0x5, 4, 2, 1}, {0x4, 7, 2, 2}, {0xb, 10, 2, 3}, {0x14, 12, 2, 4}, {0x14, 13, 2, 5},
    {0x7, 5, 3, 1}, {0x24, 8, 3, 2}, {0x1c, 12, 3, 3}, {0x13, 13, 3, 4},
    {0x6, 5, 4, 1}, {0xf, 10, 4, 2}, {0x12, 12, 4, 3}, {0x7, 6, 5, 1}, {0x9, 10, 5, 2}, {0x12, 13, 5, 3}, {0x5, 6, 6, 1}, {0x1e, 12, 6, 2},
    {0x14, 16, 6, 3},
    {0x4, 6, 7, 1}, {0x15, 12, 7, 2}, {0x7, 7, 8, 1}, {0x11, 12, 8, 2}, {0x5, 7, 9, 1}, {0x11, 13, 9, 2}, {0x27, 8, 10, 1}, {0x10, 13, 10, 2},
    {0x23, 8, 11, 1}, {0x1a, 16, 11, 2}, {0x22, 8, 12, 1}, {0x19, 16, 12, 2}, {0x20, 8, 13, 1}, {0x18, 16, 13, 2}, {0xe, 10, 14, 1},
    {0x17, 16, 14, 2}, {0xd, 10, 15, 1}, {0x16, 16, 15, 2}, {0x8, 10, 16, 1}, {0x15, 16, 16, 2},
    {0x1f, 12, 17, 1}, {0x1a, 12, 18, 1}, {0x19, 12, 19, 1}, {0x17, 12, 20, 1}, {0x16, 12, 21, 1}, {0x1f, 13, 22, 1}, {0x1e, 13, 23, 1},
    {0x1d, 13, 24, 1}, {0x1c, 13, 25, 1}, {0x1b, 13, 26, 1}, {0x1f, 16, 27, 1}, {0x1e, 16, 28, 1}, {0x1d, 16, 29, 1}, {0x1c, 16, 30, 1},
    {0x1b, 16, 31, 1},
    {0x1, 6, -2, 0}, {0x2, 2, -1, 0}};
// B-15 DCT coefficients table one
static const Mpeg2Vlc kDct1[] = {
    {0x2, 2, 0, 1}, {0x6, 3, 0, 2}, {0x7, 4, 0, 3}, {0x1c, 5, 0, 4}, {0x1d, 5, 0, 5}, {0x5, 6, 0, 6}, {0x4, 6, 0, 7}, {0x7b, 7, 0, 8},
    {0x7c, 7, 0, 9}, {0x23, 8, 0, 10}, {0x22, 8, 0, 11}, {0xfa, 8, 0, 12}, {0xfb, 8, 0, 13}, {0xfe, 8, 0, 14}, {0xff, 8, 0, 15},
    {0x1f, 14, 0, 16}, {0x1e, 14, 0, 17}, {0x1d, 14, 0, 18}, {0x1c, 14, 0, 19}, {0x1b, 14, 0, 20}, {0x1a, 14, 0, 21}, {0x19, 14, 0, 22},
    {0x18, 14, 0, 23}, {0x17, 14, 0, 24}, {0x16, 14, 0, 25}, {0x15, 14, 0, 26}, {0x14, 14, 0, 27}, {0x13, 14, 0, 28}, {0x12, 14, 0, 29},
    {0x11, 14, 0, 30}, {0x10, 14, 0, 31}, {0x18, 15, 0, 32}, {0x17, 15, 0, 33}, {0x16, 15, 0, 34}, {0x15, 15, 0, 35}, {0x14, 15, 0, 36},
    {0x13, 15, 0, 37}, {0x12, 15, 0, 38}, {0x11, 15, 0, 39}, {0x10, 15, 0, 40},
    {0x2, 3, 1, 1}, {0x6, 5, 1, 2}, {0x79, 7, 1, 3}, {0x27, 8, 1, 4}, {0x20, 8, 1, 5}, {0x16, 13, 1, 6}, {0x15, 13, 1, 7}, {0x1f, 15, 1, 8},
    {0x1e, 15, 1, 9}, {0x1d, 15, 1, 10}, {0x1c, 15, 1, 11}, {0x1b, 15, 1, 12}, {0x1a, 15, 1, 13}, {0x19, 15, 1, 14}, {0x13, 16, 1, 15},
    {0x12, 16, 1, 16}, {0x11, 16, 1, 17}, {0x10, 16, 1, 18},
    {0x5, 5, 2, 1}, {0x7, 7, 2, 2}, {0xfc, 8, 2, 3}, {0xc, 10, 2, 4}, {0x14, 13, 2, 5},
    {0x7, 5, 3, 1}, {0x26, 8, 3, 2}, {0x1c, 12, 3, 3}, {0x13, 13, 3, 4},
    {0x6, 6, 4, 1}, {0xfd, 8, 4, 2}, {0x12, 12, 4, 3}, {0x7, 6, 5, 1}, {0x4, 9, 5, 2}, {0x12, 13, 5, 3}, {0x6, 7, 6, 1}, {0x1e, 12, 6, 2},
    {0x14, 16, 6, 3},
    {0x4, 7, 7, 1}, {0x15, 12, 7, 2}, {0x5, 7, 8, 1}, {0x11, 12, 8, 2}, {0x78, 7, 9, 1}, {0x11, 13, 9, 2}, {0x7a, 7, 10, 1}, {0x10, 13, 10, 2},
    {0x21, 8, 11, 1}, {0x1a, 16, 11, 2}, {0x25, 8, 12, 1}, {0x19, 16, 12, 2}, {0x24, 8, 13, 1}, {0x18, 16, 13, 2}, {0x5, 9, 14, 1},
    {0x17, 16, 14, 2}, {0x7, 9, 15, 1}, {0x16, 16, 15, 2}, {0xd, 10, 16, 1}, {0x15, 16, 16, 2},
    {0x1f, 12, 17, 1}, {0x1a, 12, 18, 1}, {0x19, 12, 19, 1}, {0x17, 12, 20, 1}, {0x16, 12, 21, 1}, {0x1f, 13, 22, 1}, {0x1e, 13, 23, 1},
    {0x1d, 13, 24, 1}, {0x1c, 13, 25, 1}, {0x1b, 13, 26, 1}, {0x1f, 16, 27, 1}, {0x1e, 16, 28, 1}, {0x1d, 16, 29, 1}, {0x1c, 16, 30, 1},
    {0x1b, 16, 31, 1},
    {0x1, 6, -2, 0}, {0x6, 4, -1, 0}};

#define M2_N(t) (int)(sizeof(t) / sizeof(t[0]))
const Mpeg2Vlc *mpeg2_table(int which, int *n) {
    switch (which) {
    case 1: *n = M2_N(kMba); return kMba;
    case 2: *n = M2_N(kMbTypeI); return kMbTypeI;
    case 3: *n = M2_N(kMbTypeP); return kMbTypeP;
    case 4: *n = M2_N(kMbTypeB); return kMbTypeB;
    case 9: *n = M2_N(kCbp); return kCbp;
    case 10: *n = M2_N(kMotion); return kMotion;
    case 11: *n = M2_N(kDmv); return kDmv;
    case 12: *n = M2_N(kDcLuma); return kDcLuma;
    case 13: *n = M2_N(kDcChroma); return kDcChroma;
    case 14: *n = M2_N(kDct0); return kDct0;
    case 15: *n = M2_N(kDct1); return kDct1;
    }
    *n = 0; return nullptr;
}

const uint8_t kMpeg2Scan[2][64] = {
    {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63},
    {0, 8, 16, 24, 1, 9, 2, 10, 17, 25, 32, 40, 48, 56, 57, 49, 41, 33, 26, 18, 3, 11, 4, 12, 19, 27, 34, 42, 50, 58, 35, 43,
     51, 59, 20, 28, 5, 13, 6, 14, 21, 29, 36, 44, 52, 60, 37, 45, 53, 61, 22, 30, 7, 15, 23, 31, 38, 46, 54, 62, 39, 47, 55, 63}};
const uint8_t kMpeg2DefaultIntra[64] = {8, 16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38,
                                        22, 22, 26, 27, 29, 34, 37, 40, 22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58,
                                        26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83};
int mpeg2_quantiser_scale(int q_scale_type, int code) {
    static const uint8_t nl[32] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 22, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64, 72, 80, 88, 96, 104, 112};
    code &= 31;
    return q_scale_type ? nl[code] : 2 * code;
}

// ---- lookup tables built from the above ------------------------------------------------------------------------------------------------
namespace {
struct Lut {
    int maxlen = 0; const Mpeg2Vlc *t = nullptr; std::vector<uint16_t> look;     // by the next maxlen bits: (index + 1) << 5 | length; 0 = no code
    Lut(int which) {
        int n; t = mpeg2_table(which, &n);
        for (int i = 0; i < n; i++) if (t[i].len > maxlen) maxlen = t[i].len;
        look.assign((size_t)1 << maxlen, 0);
        for (int i = 0; i < n; i++) { const int sh = maxlen - t[i].len;
            for (uint32_t k = 0; k < (1u << sh); k++) look[((uint32_t)t[i].code << sh) | k] = (uint16_t)((i + 1) << 5 | t[i].len); }
    }
};
const Lut &lut(int which) {
    static const Lut l1(1), l2(2), l3(3), l4(4), l9(9), l10(10), l12(12), l13(13), l14(14), l15(15);
    switch (which) { case 1: return l1; case 2: return l2; case 3: return l3; case 4: return l4; case 9: return l9; case 10: return l10;
                     case 12: return l12; case 13: return l13; case 14: return l14; default: return l15; }
}

// B-11 has a function of its own: every call of lut() passes the guards of all its tables, and lut() is called per symbol
const Lut &lut_dmv() { static const Lut l(11); return l; }

// MSB-first bit reader over [p, p + n): bits beyond the end read as zero, and `over` says that one was consumed
struct Bits {
    const uint8_t *p; size_t nbits, pos = 0; bool over = false;
    Bits(const uint8_t *d, size_t n) : p(d), nbits(n * 8) {}
    uint32_t peek(int k) const {                     // k <= 24
        uint32_t v = 0; const size_t byte = pos >> 3;
        for (int i = 0; i < 4; i++) v = v << 8 | (byte + i < (nbits >> 3) ? p[byte + i] : 0);
        return (v << (pos & 7)) >> (32 - k);
    }
    void skip(int k) { pos += (size_t)k; if (pos > nbits) over = true; }
    uint32_t get(int k) { if (k == 0) return 0; const uint32_t v = peek(k); skip(k); return v; }
    size_t left() const { return pos < nbits ? nbits - pos : 0; }
    // one VLC symbol: the table's entry, or nullptr for an invalid code
    const Mpeg2Vlc *vlc(const Lut &l) {
        const uint16_t e = l.look[peek(l.maxlen)];
        if (!e) return nullptr;
        skip(e & 31);
        return &l.t[(e >> 5) - 1];
    }
};
}  // namespace

// ---- sequence layer ---------------------------------------------------------------------------------------------------------------------
void Mpeg2Seq::fps(long long *num, long long *den) const {
    static const int n[9] = {0, 24000, 24, 25, 30000, 30, 50, 60000, 60}, d[9] = {0, 1001, 1, 1, 1001, 1, 1, 1001, 1};
    if (frame_rate_code < 1 || frame_rate_code > 8) { *num = *den = 0; return; }
    *num = (long long)n[frame_rate_code] * (fr_ext_n + 1); *den = (long long)d[frame_rate_code] * (fr_ext_d + 1);
}
void Mpeg2Seq::sar(int *num, int *den) const {
    static const int dn[5] = {0, 1, 4, 16, 221}, dd[5] = {0, 1, 3, 9, 100};
    *num = *den = 0;
    if (aspect < 1 || aspect > 4) return;
    if (aspect == 1) { *num = *den = 1; return; }
    // the display aspect ratio belongs to the display area when a sequence_display_extension names one, else to the whole picture (6.3.3)
    const long long W = have_display && display_w ? display_w : width, H = have_display && display_h ? display_h : height;
    long long a = dn[aspect] * H, b = dd[aspect] * W, x = a, y = b;
    while (y) { const long long r = x % y; x = y; y = r; }
    if (x > 0) { a /= x; b /= x; }
    while (a > 65535 || b > 65535) { a = (a + 1) / 2; b = (b + 1) / 2; }
    *num = (int)a; *den = (int)b;
}

size_t Mpeg2Splitter::find_start(size_t from) const {
    const size_t n = in_.size();
    const uint8_t *p = in_.data();
    for (size_t i = from; i + 3 <= n;) {
        const uint8_t *q = (const uint8_t *)memchr(p + i + 2, 1, n - (i + 2));
        if (!q) return npos;
        const size_t k = (size_t)(q - p);
        if (p[k - 1] == 0 && p[k - 2] == 0) return k - 2;
        i = k - 1;
    }
    return npos;
}

static void read_matrix(Bits &b, uint8_t w[64]) { for (int k = 0; k < 64; k++) { const int v = (int)b.get(8); w[kMpeg2Scan[0][k]] = (uint8_t)(v ? v : 16); } }

// one unit behind its start code 00 00 01 `code`: n bytes at p
void Mpeg2Splitter::header_unit(int code, const uint8_t *p, size_t n) {
    Bits b(p, n);
    const int ext_id = code == 0xB5 && n >= 1 ? p[0] >> 4 : -1;
    if (expect_seq_ext_ && ext_id != 1) { refuse("MPEG-1 video (a sequence header without a sequence extension) is not supported"); return; }
    if (code == 0xB3) {                                                                     // sequence_header()
        Mpeg2Seq s;
        s.width = (int)b.get(12); s.height = (int)b.get(12); s.aspect = (int)b.get(4); s.frame_rate_code = (int)b.get(4);
        b.skip(18); const bool marker = b.get(1) != 0; b.skip(10 + 1);
        for (int k = 0; k < 64; k++) { s.w[0][k] = kMpeg2DefaultIntra[k]; s.w[1][k] = 16; }      // (every sequence header that loads none resets them)
        if (b.get(1)) read_matrix(b, s.w[0]);
        if (b.get(1)) read_matrix(b, s.w[1]);
        if (b.over || !marker || s.width == 0 || s.height == 0) { damaged_headers++; return; }
        seq_ = s; have_seq_hdr_ = true; expect_seq_ext_ = true;
        return;
    }
    if (code == 0xB5 && ext_id == 1) {                                                      // sequence_extension()
        if (!have_seq_hdr_) return;
        b.skip(4);
        seq_.profile_level = (int)b.get(8); seq_.progressive_sequence = (int)b.get(1); seq_.chroma_format = (int)b.get(2);
        if (expect_seq_ext_) { seq_.width |= (int)b.get(2) << 12; seq_.height |= (int)b.get(2) << 12; } else b.skip(4);
        b.skip(12 + 1 + 8); seq_.low_delay = (int)b.get(1); seq_.fr_ext_n = (int)b.get(2); seq_.fr_ext_d = (int)b.get(5);
        expect_seq_ext_ = false;
        if (b.over) { damaged_headers++; seq_.valid = false; return; }
        if (seq_.chroma_format == 2) { refuse("MPEG-2: chroma_format 4:2:2 is not supported"); return; }
        if (seq_.chroma_format == 3) { refuse("MPEG-2: chroma_format 4:4:4 is not supported"); return; }
        if (seq_.chroma_format != 1) { damaged_headers++; seq_.valid = false; return; }
        if (seq_.height > 2800) { refuse("MPEG-2: slice_vertical_position_extension (a picture of more than 2800 lines) is not supported"); return; }
        seq_.valid = true;
        return;
    }
    if (code == 0xB5 && (ext_id == 5 || ext_id == 9 || ext_id == 10)) { refuse("MPEG-2: the scalable extensions are not supported"); return; }
    if (code == 0xB5 && ext_id == 2) {                                                      // sequence_display_extension()
        b.skip(4 + 3);
        Mpeg2Seq s = seq_;
        s.have_display = true; s.have_colour = b.get(1) != 0;
        if (s.have_colour) { s.primaries = (int)b.get(8); s.transfer = (int)b.get(8); s.matrix = (int)b.get(8); }
        s.display_w = (int)b.get(14); b.skip(1); s.display_h = (int)b.get(14);
        if (b.over) damaged_headers++; else seq_ = s;
        return;
    }
    if (code == 0xB5 && ext_id == 3) {                                                      // quant_matrix_extension()
        b.skip(4);
        uint8_t w[4][64]; bool load[4];
        for (int i = 0; i < 4; i++) { load[i] = b.get(1) != 0; if (load[i]) read_matrix(b, w[i]); }
        if (b.over) { damaged_headers++; return; }
        for (int i = 0; i < 2; i++) if (load[i]) memcpy(seq_.w[i], w[i], 64);               // (the chroma matrices belong to 4:2:2 / 4:4:4)
        return;
    }
    if (code == 0x00) {                                                                     // picture_header()
        Mpeg2Pic pc;
        pc.temporal_reference = (int)b.get(10); pc.type = (int)b.get(3); b.skip(16);
        if (pc.type == 2 || pc.type == 3) b.skip(4);                                        // (full_pel_forward_vector, forward_f_code: MPEG-1's)
        if (pc.type == 3) b.skip(4);
        if (b.over) { damaged_headers++; return; }
        if (pc.type == 4) { refuse("MPEG-2: D pictures are not supported"); return; }
        if (pc.type < 1 || pc.type > 3) { damaged_headers++; return; }
        pic_ = pc; in_pic_ = true;
        return;
    }
    if (code == 0xB5 && ext_id == 8) {                                                      // picture_coding_extension()
        if (!in_pic_) return;
        b.skip(4);
        for (int s = 0; s < 2; s++) for (int t = 0; t < 2; t++) pic_.f_code[s][t] = (int)b.get(4);
        pic_.intra_dc_precision = (int)b.get(2); pic_.picture_structure = (int)b.get(2); pic_.top_field_first = (int)b.get(1);
        pic_.frame_pred_frame_dct = (int)b.get(1); pic_.concealment_mv = (int)b.get(1); pic_.q_scale_type = (int)b.get(1);
        pic_.intra_vlc_format = (int)b.get(1); pic_.alternate_scan = (int)b.get(1); pic_.repeat_first_field = (int)b.get(1);
        b.skip(1); pic_.progressive_frame = (int)b.get(1);
        if (b.over) { damaged_headers++; in_pic_ = false; return; }
        if ((pic_.picture_structure == 1 || pic_.picture_structure == 2) && !field_pictures) {
            refuse("MPEG-2: field pictures are not supported (option mpeg2_field_pictures decodes them)"); return; }
        if (pic_.picture_structure == 0) { damaged_headers++; in_pic_ = false; return; }
        pic_.have_ext = true; pic_.field_pictures = field_pictures;
        return;
    }
    if (code >= 0x01 && code <= 0xAF && in_pic_ && !pic_.have_ext)
        refuse("MPEG-1 video (a picture without a picture coding extension) is not supported");
    // group_of_pictures_header, user_data, sequence_end, the display / copyright extensions: nothing to keep
}

// ---- slices -----------------------------------------------------------------------------------------------------------------------------
namespace {
// EXT = the picture's handle has option mpeg2_field_pictures on.  EXT = false is the slice decode of before the option, to the instruction: every
// branch on field pictures, 16x8 and dual prime is compiled out of it (fp() is false, frame_motion_type 3 is refused), so a handle at option 0
// pays nothing for them -- this loop runs once per macroblock of every stream
template <bool EXT> struct SliceDec {
    const Mpeg2Pic &pic; Mpeg2Jobs &jobs; std::vector<uint8_t> &covered;
    int mb_w, mb_h, W, H;              // of the picture: a field picture's mb_h and H are the field's
    bool fieldpic_; int par;           // a field picture, and its parity (0 top, 1 bottom)
    bool fp() const { return EXT && fieldpic_; }
    int pmv[2][2][2], dc_pred[3], qscale = 2;
    uint16_t prev_dir = M2_FWD;
    bool refuse = false; std::string err;

    void reset_dc() { dc_pred[0] = dc_pred[1] = dc_pred[2] = 1 << (pic.intra_dc_precision + 7); }
    void reset_pmv() { memset(pmv, 0, sizeof pmv); }
    bool bad(const char *what) { if (err.empty()) err = std::string("MPEG-2: ") + what; return false; }

    // 7.6.3.1: one component from its predictor
    bool mv_component(Bits &b, int f_code, int pred, int *out) {
        if (f_code < 1 || f_code > 9) return bad("an f_code outside 1..9 is used");
        const Mpeg2Vlc *m = b.vlc(lut(10));
        if (!m) return bad("invalid motion_code");
        int delta = 0;
        if (m->a) {
            const bool neg = b.get(1) != 0;
            const int r_size = f_code - 1;
            delta = ((m->a - 1) << r_size) + (int)b.get(r_size) + 1;
            if (neg) delta = -delta;
        }
        const int f = 1 << (f_code - 1), lo = -16 * f, hi = 16 * f - 1;
        int v = pred + delta;
        if (v < lo) v += 32 * f; else if (v > hi) v -= 32 * f;
        *out = v;
        return true;
    }
    // motion_vectors(s): the vectors land in rec.mv[2 s + r] and the predictors move as Table 7-9 / 7.6.3.4 say.  Table 7-12 / 7-13 by mode:
    // kFrame one vector; kField2 field prediction in a frame picture: two vectors with their selects, the vertical predictor halved and stored back
    // doubled; kField field prediction in a field picture: one vector with its select; k16x8: two such; kDual one vector without select, a dmvector
    // behind each component's residual (in a frame picture the vertical predictor is halved, as for kField2).
    // X = false knows kFrame and kField2 only: the instantiation the macroblocks of frame pictures without dual prime run, which compiles to the
    // routine of before option mpeg2_field_pictures (this loop is per macroblock of every stream); X = true knows every mode
    enum { kFrame, kField2, kField, k16x8, kDual };
    template <bool X> bool motion_vectors(Bits &b, int s, int mode, Mpeg2Mb &rec, int dmv[2] = nullptr) {
        const bool dual = X && mode == kDual, two = mode == kField2 || (X && mode == k16x8);
        const bool sel = mode == kField2 || (X && (mode == kField || mode == k16x8)), half = mode == kField2 || (dual && !fp());
        for (int r = 0; r < (two ? 2 : 1); r++) {
            if (sel) rec.flags |= (uint16_t)(b.get(1) << (M2_SEL_SHIFT + 2 * s + r));
            int x = 0, y = 0;
            if (!mv_component(b, pic.f_code[s][0], pmv[r][s][0], &x)) return false;
            if (dual) { const Mpeg2Vlc *d = b.vlc(lut_dmv()); if (!d) return bad("invalid dmvector"); dmv[0] = d->a; }
            if (!mv_component(b, pic.f_code[s][1], half ? pmv[r][s][1] >> 1 : pmv[r][s][1], &y)) return false;
            if (dual) { const Mpeg2Vlc *d = b.vlc(lut_dmv()); if (!d) return bad("invalid dmvector"); dmv[1] = d->a; }
            pmv[r][s][0] = x; pmv[r][s][1] = half ? y * 2 : y;
            rec.mv[2 * s + r][0] = (int16_t)x; rec.mv[2 * s + r][1] = (int16_t)y;
        }
        if (!two) { pmv[1][s][0] = pmv[0][s][0]; pmv[1][s][1] = pmv[0][s][1]; }
        return true;
    }
    // 7.6.3.6: the vectors of the opposite parity from the transmitted one (in rec.mv[0]) and dmvector
    void derive_dual(Mpeg2Mb &rec, const int dmv[2]) {
        const int vx = rec.mv[0][0], vy = rec.mv[0][1];
        auto put = [&](int slot, int m, int e) {           // (mpeg2_vlc.h: the arithmetic the device-VLC lane runs too)
            int x, y; mpeg2_dual_vector(vx, vy, dmv[0], dmv[1], m, e, &x, &y);
            rec.mv[slot][0] = (int16_t)x; rec.mv[slot][1] = (int16_t)y;
        };
        if (fp()) put(2, 1, par ? 1 : -1);                                     // the field predicted: top -1, bottom +1
        else { put(2, pic.top_field_first ? 1 : 3, -1); put(3, pic.top_field_first ? 3 : 1, 1); }      // [2] the top lines, [3] the bottom lines
    }
    // the select bits of "the field of the picture's own parity" for both directions (0 in a frame picture)
    uint16_t own_parity() const { return fp() ? (uint16_t)(par << M2_SEL_SHIFT | par << (M2_SEL_SHIFT + 2)) : (uint16_t)0; }
    // the standard forbids vectors that reach outside the reference picture; a hostile stream does not: clamp, mark, count.  Each vector's block --
    // 16 lines of the frame; 8 lines of a field of it (field and dual-prime vectors of a frame picture); 16 lines of the reference field (a field
    // picture); 8 of them for each 16x8 vector -- stays inside what it reads from.  X as for motion_vectors: false = a frame picture's record
    // without dual prime
    template <bool X> void clamp_vectors(Mpeg2Mb &rec, int mx, int my) {
        if (rec.flags & M2_INTRA) return;
        const bool field = (rec.flags & M2_FIELD_MV) != 0, dual = X && (rec.flags & M2_DUAL) != 0, m16x8 = X && (rec.flags & M2_16X8) != 0, fp = X && fieldpic_;
        bool cl = false;
        auto one = [&](int slot, int r) {
            int16_t *v = rec.mv[slot];
            const int x_lo = -2 * mx * 16, x_hi = 2 * (W - 16 - mx * 16);
            const int pos = fp ? my * 16 + (m16x8 ? 8 * r : 0) : (field || dual ? my * 8 : my * 16);
            const int span = fp ? (m16x8 ? 8 : 16) : (field || dual ? 8 : 16), size = !fp && (field || dual) ? H / 2 : H;
            const int y_lo = -2 * pos, y_hi = 2 * (size - span - pos);
            const int x = v[0] < x_lo ? x_lo : (v[0] > x_hi ? x_hi : v[0]), y = v[1] < y_lo ? y_lo : (v[1] > y_hi ? y_hi : v[1]);
            if (x != v[0] || y != v[1]) { cl = true; v[0] = (int16_t)x; v[1] = (int16_t)y; }
        };
        if (dual) { one(0, 0); one(2, 0); if (!fp) one(3, 0); }
        else for (int s = 0; s < 2; s++) {
            if (!(rec.flags & (s ? M2_BWD : M2_FWD))) continue;
            for (int r = 0; r < (field || m16x8 ? 2 : 1); r++) one(2 * s + r, r);
        }
        if (cl) { rec.flags |= M2_CLAMPED; jobs.clamped++; }
    }
    // 7.2: one block's levels into the entry list
    bool block(Bits &b, int k, bool intra, Mpeg2Mb &rec) {
        const size_t e0 = jobs.entries.size();
        int n = 0;
        if (intra) {
            const Mpeg2Vlc *d = b.vlc(lut(k < 4 ? 12 : 13));
            if (!d) return bad("invalid dct_dc_size");
            int diff = 0;
            if (d->a) { const int v = (int)b.get(d->a), half = 1 << (d->a - 1); diff = v >= half ? v : v + 1 - 2 * half; }
            int &pred = dc_pred[k < 4 ? 0 : k - 3];
            pred += diff;
            if (pred < 0 || pred >= (1 << (8 + pic.intra_dc_precision))) return bad("an intra DC coefficient out of range");
            if (pred) jobs.entries.push_back((uint32_t)pred << 16);
            n = 1;
        }
        const Lut &l = lut(intra && pic.intra_vlc_format ? 15 : 14);
        const uint8_t *scan = kMpeg2Scan[pic.alternate_scan ? 1 : 0];
        for (;;) {
            int run, level;
            if (!intra && n == 0 && b.peek(1)) { b.skip(1); run = 0; level = b.get(1) ? -1 : 1; }
            else {
                const Mpeg2Vlc *c = b.vlc(l);
                if (!c) return bad("invalid DCT coefficient code");
                if (c->a == -1) { if (!intra && n == 0) return bad("an empty coded block"); break; }
                if (c->a == -2) {
                    run = (int)b.get(6); level = (int)b.get(12); if (level >= 2048) level -= 4096;
                    if (level == 0 || level == -2048) return bad("a forbidden escape level");
                } else { run = c->a; level = b.get(1) ? -c->b : c->b; }
            }
            n += run;
            if (n > 63 || b.over) return bad("a block with more than 64 coefficients");
            jobs.entries.push_back((uint32_t)scan[n] | (uint32_t)(uint16_t)(int16_t)level << 16);
            n++;
        }
        rec.count[k] = (uint8_t)(jobs.entries.size() - e0);
        return true;
    }
    void put(int addr, const Mpeg2Mb &rec) {
        Mpeg2Mb r = rec;
        if (EXT && (fieldpic_ || (r.flags & M2_DUAL))) {
            clamp_x(r, addr % mb_w, addr / mb_w);
            if (r.flags & M2_16X8) jobs.n_16x8++;
            if (r.flags & M2_DUAL) jobs.n_dual++;
        } else clamp_vectors<false>(r, addr % mb_w, addr / mb_w);
        jobs.mbs[(size_t)addr] = r; covered[(size_t)addr] = 1;
    }
    void skipped(int addr) {
        Mpeg2Mb rec = {};
        rec.first = (uint32_t)jobs.entries.size(); rec.qscale = (uint8_t)qscale;
        reset_dc();
        if (pic.type == 2) { reset_pmv(); rec.flags = M2_FWD | own_parity(); }      // (a field picture: from the field of its own parity)
        else {                                                    // B: the direction(s) of the macroblock before it, frame prediction from the predictors
            rec.flags = prev_dir | own_parity();                  // (a field picture: field prediction from the same-parity field(s))
            for (int s = 0; s < 2; s++) { rec.mv[2 * s][0] = (int16_t)pmv[0][s][0]; rec.mv[2 * s][1] = (int16_t)pmv[0][s][1]; }
        }
        put(addr, rec);
    }
    // One macroblock (6.2.5).  FP = a field picture: field_motion_type with every forward or backward macroblock, no dct_type, a field select with
    // every vector but dual prime's, the concealment vector included.  FP = false, a frame picture, is the routine of before option
    // mpeg2_field_pictures with one branch more: frame_motion_type 3 goes to the vector routine that knows dual prime
    // (the instantiations only field pictures and dual prime reach are called through these, out of line: the frame-picture path keeps its size)
    __attribute__((noinline)) bool macroblock_field(Bits &b, int addr) { return macroblock_t<true>(b, addr); }
    __attribute__((noinline)) bool vectors_x(Bits &b, int s, int mode, Mpeg2Mb &rec, int dmv[2]) { return motion_vectors<true>(b, s, mode, rec, dmv); }
    __attribute__((noinline)) void clamp_x(Mpeg2Mb &rec, int mx, int my) { clamp_vectors<true>(rec, mx, my); }
    bool macroblock(Bits &b, int addr) { return fp() ? macroblock_field(b, addr) : macroblock_t<false>(b, addr); }
    template <bool FP> bool macroblock_t(Bits &b, int addr) {
        const Mpeg2Vlc *t = b.vlc(lut(pic.type == 1 ? 2 : (pic.type == 2 ? 3 : 4)));
        if (!t) return bad("invalid macroblock_type");
        const int ty = t->a;
        const bool quant = ty & 1, mf = (ty & 2) != 0, mb = (ty & 4) != 0, pattern = (ty & 8) != 0, intra = (ty & 16) != 0;
        bool field_dct = false;
        int mode = FP ? kField : kFrame;
        if (FP) {
            if (mf || mb) {
                const int fmt = (int)b.get(2);                     // field_motion_type: always present
                if (fmt == 0) return bad("reserved field_motion_type");
                mode = fmt == 1 ? kField : (fmt == 2 ? k16x8 : kDual);
            }
        } else if ((mf || mb) && !pic.frame_pred_frame_dct) {
            const int fmt = (int)b.get(2);                         // frame_motion_type
            if (fmt == 3 && !EXT) { refuse = true; return bad("dual-prime prediction is not supported"); }
            if (fmt == 0) return bad("reserved frame_motion_type");
            mode = fmt == 1 ? kField2 : (fmt == 2 || !EXT ? kFrame : kDual);
        }
        if (EXT && mode == kDual && (pic.type != 2 || !mf)) return bad("dual-prime prediction in a B picture");
        if (!FP && !pic.frame_pred_frame_dct && (intra || pattern)) field_dct = b.get(1) != 0;
        if (quant) { const int c = (int)b.get(5); if (c == 0) return bad("quantiser_scale_code 0"); qscale = mpeg2_quantiser_scale(pic.q_scale_type, c); }
        Mpeg2Mb rec = {};
        rec.first = (uint32_t)jobs.entries.size(); rec.qscale = (uint8_t)qscale;
        if (field_dct) rec.flags |= M2_FIELD_DCT;
        if (intra) {
            rec.flags |= M2_INTRA;
            if (pic.concealment_mv) {                              // parsed, with their marker bit; they move the predictors and are otherwise unused
                Mpeg2Mb scratch = {};
                if (!(FP ? vectors_x(b, 0, kField, scratch, nullptr) : motion_vectors<false>(b, 0, kFrame, scratch))) return false;
                if (!b.get(1)) return bad("the marker bit behind concealment vectors is 0");
            } else reset_pmv();
        } else {
            reset_dc();
            if (FP || (EXT && mode == kDual)) {
                int dmv[2] = {0, 0};
                if (mf) { rec.flags |= M2_FWD; if (!vectors_x(b, 0, mode, rec, dmv)) return false; }
                if (mb) { rec.flags |= M2_BWD; if (!vectors_x(b, 1, mode, rec, dmv)) return false; }
                if (mode == k16x8) rec.flags |= M2_16X8;
                if (mode == kDual) { rec.flags |= M2_DUAL; derive_dual(rec, dmv); }
            } else {
                if (mf) { rec.flags |= M2_FWD; if (!motion_vectors<false>(b, 0, mode, rec)) return false; }
                if (mb) { rec.flags |= M2_BWD; if (!motion_vectors<false>(b, 1, mode, rec)) return false; }
                if (mode == kField2) rec.flags |= M2_FIELD_MV;
            }
            if (!mf && !mb) { if (pic.type != 2) return bad("a macroblock without prediction in a B picture"); rec.flags |= M2_FWD | (FP ? own_parity() : 0); reset_pmv(); }
            prev_dir = rec.flags & (M2_FWD | M2_BWD);
        }
        int cbp = intra ? 63 : 0;
        if (pattern) { const Mpeg2Vlc *c = b.vlc(lut(9)); if (!c || c->a == 0) return bad("invalid coded_block_pattern"); cbp = c->a; }
        rec.cbp = (uint8_t)cbp;
        for (int k = 0; k < 6; k++) if (cbp & (32 >> k)) { if (!block(b, k, intra, rec)) return false; }
        if (b.over) return bad("a slice ends inside a macroblock");
        put(addr, rec);
        return true;
    }
    // one slice: p = the bytes behind its start code, vpos = slice_vertical_position
    void slice(const uint8_t *p, size_t n, int vpos) {
        Bits b(p, n);
        const int row = vpos - 1;
        if (row < 0 || row >= mb_h) { bad("a slice outside the picture"); return; }
        { const int c = (int)b.get(5); if (c == 0) { bad("quantiser_scale_code 0"); return; } qscale = mpeg2_quantiser_scale(pic.q_scale_type, c); }
        if (b.get(1)) { b.skip(8); while (b.get(1) && !b.over) b.skip(8); }       // intra_slice_flag, intra_slice, reserved_bits, extra_information_slice
        reset_dc(); reset_pmv(); prev_dir = M2_FWD;
        int prev = row * mb_w - 1; bool first = true;
        while (!b.over && b.left() > 0 && b.peek(23) != 0) {
            int inc = 0;
            for (;;) {
                const Mpeg2Vlc *m = b.vlc(lut(1));
                if (!m) { bad("invalid macroblock_address_increment"); return; }
                if (m->a == 34) { inc += 33; continue; }
                inc += m->a; break;
            }
            const int addr = prev + inc;
            if (addr >= mb_w * mb_h) { bad("a macroblock address beyond the picture"); return; }
            if (!first && inc > 1) {
                if (pic.type == 1) { bad("a skipped macroblock in an I picture"); return; }
                for (int a = prev + 1; a < addr; a++) skipped(a);
            }
            const size_t e0 = jobs.entries.size();
            if (!macroblock(b, addr)) { jobs.entries.resize(e0); return; }
            prev = addr; first = false;
        }
    }
};
}  // namespace

// (each instantiation out of line, so that option 0 runs a body of its own, laid out as before)
template <bool EXT> static __attribute__((noinline)) std::string decode_picture_t(const Mpeg2Pic &pic, Mpeg2Jobs &jobs, bool *refuse) {
    const int mb_w = pic.seq.mb_w(), mb_h = pic.mb_h();
    jobs.mbs.assign((size_t)mb_w * mb_h, Mpeg2Mb{}); jobs.entries.clear(); jobs.clamped = 0; jobs.n_16x8 = jobs.n_dual = 0;
    std::vector<uint8_t> covered((size_t)mb_w * mb_h, 0);
    SliceDec<EXT> d{pic, jobs, covered, mb_w, mb_h, mb_w * 16, mb_h * 16, pic.field(), pic.picture_structure == 2 ? 1 : 0, {}, {}, 2, M2_FWD, false, std::string()};
    // the picture's data: units 00 00 01 vpos ...; each runs up to the next one (the splitter cut them at start codes, so none hides inside)
    const uint8_t *p = pic.data.data(); const size_t n = pic.data.size();
    size_t o = 0;
    while (o + 4 <= n) {
        size_t e = o + 4;
        while (e + 3 <= n && !(p[e] == 0 && p[e + 1] == 0 && p[e + 2] == 1)) e++;
        if (e + 3 > n) e = n;
        d.slice(p + o + 4, e - (o + 4), p[o + 3]);
        if (d.refuse) { *refuse = true; return d.err; }
        o = e;
    }
    // macroblocks no slice covers: zero-vector forward copies (P, B; a field picture: of the field of its own parity), grey intra blocks (I)
    bool holes = false;
    for (size_t a = 0; a < covered.size(); a++) if (!covered[a]) {
        holes = true;
        Mpeg2Mb rec = {};
        rec.first = (uint32_t)jobs.entries.size(); rec.qscale = 2;
        if (pic.type == 1) { rec.flags = M2_INTRA; rec.cbp = 63;
            for (int k = 0; k < 6; k++) { jobs.entries.push_back((uint32_t)(128 << pic.intra_dc_precision) << 16); rec.count[k] = 1; } }
        else rec.flags = M2_FWD | d.own_parity();
        jobs.mbs[a] = rec;
    }
    if (holes && d.err.empty()) d.err = "MPEG-2: macroblocks that no slice covers";
    return d.err;
}

std::string mpeg2_decode_picture(const Mpeg2Pic &pic, Mpeg2Jobs &jobs, bool *refuse) {
    return pic.field_pictures ? decode_picture_t<true>(pic, jobs, refuse) : decode_picture_t<false>(pic, jobs, refuse);
}

// ---- option mpeg2_device_vlc -----------------------------------------------------------------------------------------------------------
namespace {
// one-level table of mpeg2_vlc.h: by the next `bits` bits, length | (a + 1) << 5
bool fill_small(int which, uint16_t *look, int bits) {
    int n; const Mpeg2Vlc *t = mpeg2_table(which, &n);
    for (int i = 0; i < (1 << bits); i++) look[i] = 0;
    for (int i = 0; i < n; i++) {
        if (t[i].len > bits || t[i].a < 0 || t[i].a > 2046) return false;
        const int sh = bits - t[i].len;
        for (uint32_t k = 0; k < (1u << sh); k++) look[((uint32_t)t[i].code << sh) | k] = (uint16_t)(t[i].len | (t[i].a + 1) << 5);
    }
    return true;
}
// two-level table of B-14 / B-15: (length - 1) | run << 4 | level << 10, run 62 = escape, 63 = end of block
bool fill_dct(int which, uint16_t *look) {
    int n; const Mpeg2Vlc *t = mpeg2_table(which, &n);
    for (int i = 0; i < 1280; i++) look[i] = 0;
    for (int i = 0; i < n; i++) {
        const int len = t[i].len, run = t[i].a == -1 ? 63 : (t[i].a == -2 ? 62 : t[i].a), level = t[i].a < 0 ? 0 : t[i].b;
        if (len < 1 || len > 16 || run < 0 || run > 63 || (t[i].a >= 0 && run > 61) || level < 0 || level > 63) return false;
        const uint16_t e = (uint16_t)((len - 1) | run << 4 | level << 10);
        const uint32_t c16 = (uint32_t)t[i].code << (16 - len);              // the code at the top of 16 bits
        if (c16 >> 10) {                                                     // level 1: one of its first six bits is set
            if (len > 8) return false;
            for (uint32_t k = 0; k < (1u << (8 - len)); k++) look[(c16 >> 8) | k] = e;
        } else {
            for (uint32_t k = 0; k < (1u << (16 - len)); k++) look[256 + ((c16 | k) & 1023)] = e;
        }
    }
    return true;
}
}  // namespace

const Mpeg2VlcTables *mpeg2_vlc_tables() {
    static Mpeg2VlcTables tab;
    static const bool ok = [] {
        bool good = fill_small(1, tab.mba, 11) && fill_small(2, tab.mbtype[0], 6) && fill_small(3, tab.mbtype[1], 6) && fill_small(4, tab.mbtype[2], 6) &&
                    fill_small(9, tab.cbp, 9) && fill_small(10, tab.motion, 10) && fill_small(12, tab.dc_luma, 9) && fill_small(13, tab.dc_chroma, 10) &&
                    fill_dct(14, tab.dct[0]) && fill_dct(15, tab.dct[1]);
        memcpy(tab.scan, kMpeg2Scan, sizeof tab.scan);
        for (int ty = 0; ty < 2; ty++) for (int c = 0; c < 32; c++) tab.qscale[ty][c] = (uint8_t)mpeg2_quantiser_scale(ty, c);
        return good;
    }();
    return ok ? &tab : nullptr;
}

Mpeg2VlcPic mpeg2_vlc_pic(const Mpeg2Pic &pic) {
    Mpeg2VlcPic v = {};
    v.type = pic.type;
    for (int s = 0; s < 2; s++) for (int t = 0; t < 2; t++) v.f_code[s][t] = pic.f_code[s][t];
    v.intra_dc_precision = pic.intra_dc_precision; v.frame_pred_frame_dct = pic.frame_pred_frame_dct; v.concealment_mv = pic.concealment_mv;
    v.q_scale_type = pic.q_scale_type; v.intra_vlc_format = pic.intra_vlc_format; v.alternate_scan = pic.alternate_scan;
    v.mb_w = pic.seq.mb_w(); v.mb_h = pic.seq.mb_h();
    v.dual_prime = pic.field_pictures ? 1 : 0; v.top_field_first = pic.top_field_first;
    return v;
}

std::string mpeg2_slice_scan(const Mpeg2Pic &pic, Mpeg2SliceScan &out) {
    const int mb_w = pic.seq.mb_w(), mb_h = pic.seq.mb_h();
    const uint32_t total = (uint32_t)mb_w * (uint32_t)mb_h;
    out.slices.clear(); out.bytes.clear(); out.n_entries = 0;
    const uint8_t *p = pic.data.data(); const size_t n = pic.data.size();
    size_t o = 0;
    while (o + 4 <= n) {
        // the next start code prefix 00 00 01 at or behind o + 4 (memchr for the 01, as Mpeg2Splitter::find_start looks for it)
        size_t e = n;
        for (size_t i = o + 6; i < n;) {
            const uint8_t *q = (const uint8_t *)memchr(p + i, 1, n - i);
            if (!q) break;
            const size_t k = (size_t)(q - p);
            if (p[k - 1] == 0 && p[k - 2] == 0) { e = k - 2; break; }
            i = k + 1;
        }
        const uint8_t *sp = p + o + 4; const size_t L = e - (o + 4);
        const int row = (int)p[o + 3] - 1;
        o = e;
        if (row < 0 || row >= mb_h) return "MPEG-2: a slice outside the picture";
        Bits b(sp, L);
        if (b.get(5) == 0) return "MPEG-2: quantiser_scale_code 0";
        if (b.get(1)) { b.skip(8); while (b.get(1) && !b.over) b.skip(8); }
        if (b.over || b.left() == 0 || b.peek(23) == 0) continue;            // no macroblock: the slice decode's loop would not run once
        uint32_t inc = 0;
        for (;;) {
            const Mpeg2Vlc *m = b.vlc(lut(1));
            if (!m) return "MPEG-2: invalid macroblock_address_increment";
            if (m->a == 34) { inc += 33; if (inc > total) return "MPEG-2: a macroblock address beyond the picture"; continue; }
            inc += (uint32_t)m->a; break;
        }
        const uint32_t s = (uint32_t)row * (uint32_t)mb_w + inc - 1;
        if (s >= total) return "MPEG-2: a macroblock address beyond the picture";
        Mpeg2Slice sl = {};                                                  // (lo holds the first address until the table is complete)
        sl.byte_off = (uint32_t)out.bytes.size(); sl.n_bytes = (uint32_t)L; sl.row = (uint32_t)row; sl.lo = s;
        if (!out.slices.empty() && s <= out.slices.back().lo) return "MPEG-2: slices that overlap or are out of order";
        out.slices.push_back(sl);
        out.bytes.insert(out.bytes.end(), sp, sp + L);
        out.bytes.resize(sl.byte_off + mpeg2_vlc_padded((uint32_t)L), 0);
    }
    if (out.slices.empty()) return "MPEG-2: a picture without slices";
    uint64_t first_entry = 0;
    for (size_t i = 0; i < out.slices.size(); i++) {
        Mpeg2Slice &sl = out.slices[i];
        sl.hi = i + 1 < out.slices.size() ? out.slices[i + 1].lo : total;
        if (i == 0) sl.lo = 0;
    }
    for (auto &sl : out.slices) {
        sl.first_entry = (uint32_t)first_entry; sl.entry_cap = mpeg2_vlc_capacity(sl.n_bytes, sl.hi - sl.lo);
        first_entry += sl.entry_cap;
    }
    if (first_entry > 0x7fffffffull) return "MPEG-2: a picture whose entry list would not fit";
    out.n_entries = (uint32_t)first_entry;
    return std::string();
}

}  // namespace jmamd
