// tools/pichash_asan.cpp -- the lane routines of k_hevc_pichash (jmcodec_amd/csrc/pichash_packed.h) walked on the CPU, built with AddressSanitizer /
// UBSan (host sanitizers; `make -C tools pichash_asan`).  Every surface is a heap buffer of exactly the bytes the hashes cover -- the last row ends
// with the allocation -- so a read past a row's samples aborts.  The results are compared with the two definitions written out below: the bit-serial
// CRC of INTEGRATION.md "Picture hash" and the plain checksum loop.  Nothing here touches a device.
//   pichash_asan                      the walk; prints "ok: ..." and returns 0
//   pichash_asan shift r n [r n ...]  prints r * x^(8 n) mod P (hexadecimal), one line per pair: the routine that places a chunk's CRC in a picture
#include "../jmcodec_amd/csrc/pichash_packed.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace jmamd;

// ---- the definitions -----------------------------------------------------------------------------------------------------------------------------
static uint32_t crc_bit_serial(const std::vector<uint8_t> &data) {
    uint32_t crc = 0xFFFF;
    auto bit = [&](uint32_t b) { const bool msb = (crc & 0x8000u) != 0; crc = ((crc << 1) + b) & 0xFFFFu; if (msb) crc ^= 0x1021u; };
    for (uint8_t v : data) for (int k = 7; k >= 0; k--) bit((v >> k) & 1u);
    for (int k = 0; k < 16; k++) bit(0);
    return crc;
}
static uint32_t checksum_plain(const std::vector<uint8_t> &plane, int w, int h) {
    uint32_t sum = 0;
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) sum += (uint32_t)(plane[(size_t)y * w + x] ^ (uint8_t)((x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8)));
    return sum;
}
static uint32_t mul_x(uint32_t a) { a <<= 1; return (a & 0x10000u) ? (a ^ 0x11021u) : a; }            // a * x mod P, one bit at a time
static uint32_t mul_bitwise(uint32_t a, uint32_t b) { uint32_t r = 0; for (int i = 15; i >= 0; i--) { r = mul_x(r); if ((b >> i) & 1u) r ^= a; } return r; }

static int fail(const char *what, long a = 0, long b = 0) { fprintf(stderr, "FAILED: %s (%ld, %ld)\n", what, a, b); return 1; }

// ---- one surface: every work item of every band, as the kernel runs them ------------------------------------------------------------------------
static int walk(int w, int h, int pitch, unsigned seed, int fill, const uint16_t *lo, const uint16_t *hi, int &walks) {
    const int chroma_offset = pitch * h;
    const size_t bytes = (size_t)chroma_offset + (size_t)pitch * (h / 2 - 1) + w;               // ends with the last chroma row's last sample
    std::unique_ptr<uint8_t[]> surf(new uint8_t[bytes]);
    unsigned s = seed;
    for (size_t i = 0; i < bytes; i++) { s = s * 1664525u + 1013904223u; surf[i] = fill >= 0 ? (uint8_t)fill : (uint8_t)(s >> 24); }
    std::vector<uint8_t> Y((size_t)w * h), Cb((size_t)(w / 2) * (h / 2)), Cr(Cb.size());
    for (int y = 0; y < h; y++) memcpy(&Y[(size_t)y * w], &surf[(size_t)y * pitch], w);
    for (int y = 0; y < h / 2; y++) for (int x = 0; x < w / 2; x++) {
        Cb[(size_t)y * (w / 2) + x] = surf[(size_t)chroma_offset + (size_t)y * pitch + 2 * x];
        Cr[(size_t)y * (w / 2) + x] = surf[(size_t)chroma_offset + (size_t)y * pitch + 2 * x + 1]; }
    for (int wide = 0; wide < 2; wide++) {
        if (wide && ((((uintptr_t)surf.get()) | (uintptr_t)pitch | (uintptr_t)chroma_offset) & 15)) continue;
        ph::Acc a;
        for (int band = 0; band < ph::band_count(h); band++)
            for (int i = 0; i < ph::band_items(w, h, band); i++) ph::hash_item(surf.get(), pitch, chroma_offset, w, h, band, i, wide != 0, lo, hi, a);
        const uint32_t cbytes = (uint32_t)(w / 2) * (uint32_t)(h / 2);
        a.crc_y ^= ph::init_term((uint32_t)w * (uint32_t)h, lo, hi); a.crc_cb ^= ph::init_term(cbytes, lo, hi); a.crc_cr ^= ph::init_term(cbytes, lo, hi);
        if (a.crc_y != crc_bit_serial(Y) || a.crc_cb != crc_bit_serial(Cb) || a.crc_cr != crc_bit_serial(Cr)) return fail("CRC of a surface", w, h);
        if (a.sum_y != checksum_plain(Y, w, h) || a.sum_cb != checksum_plain(Cb, w / 2, h / 2) || a.sum_cr != checksum_plain(Cr, w / 2, h / 2))
            return fail("checksum of a surface", w, h);
        walks++;
    }
    return 0;
}

int main(int argc, char **argv) {
    static uint16_t lo[ph::kPowLo], hi[ph::kPowHi];
    ph::fill_pow_tables(lo, hi);
    if (argc >= 2 && !strcmp(argv[1], "shift")) {
        for (int k = 2; k + 1 < argc; k += 2)
            printf("%04x\n", ph::shift_bytes((uint32_t)strtoul(argv[k], nullptr, 0) & 0xFFFFu, (uint32_t)strtoul(argv[k + 1], nullptr, 0), lo, hi));
        return 0;
    }
    // the byte step against the bit-serial form: the catalogue check value of CRC-16/SPI-FUJITSU, then random strings
    {
        const char *t = "123456789";
        std::vector<uint8_t> v(t, t + 9);
        uint32_t c = ph::kCrcInit;
        for (uint8_t b : v) c = ph::crc_byte(c, b);
        if (c != 0xE5CCu || crc_bit_serial(v) != 0xE5CCu) return fail("check value 0xE5CC", (long)c, (long)crc_bit_serial(v));
        unsigned s = 7;
        for (int n = 0; n < 300; n++) {
            std::vector<uint8_t> d((size_t)n);
            for (auto &b : d) { s = s * 1664525u + 1013904223u; b = (uint8_t)(s >> 24); }
            c = ph::kCrcInit;
            for (uint8_t b : d) c = ph::crc_byte(c, b);
            if (c != crc_bit_serial(d)) return fail("byte step against the bit-serial CRC", n);
        }
    }
    // powers of x: the table, the order of x, the product, xpow and the two-table form
    {
        uint32_t sq = 2;
        for (int k = 0; k < 15; k++) { if (ph::kXPow2[k] != sq) return fail("kXPow2", k); sq = mul_bitwise(sq, sq); }
        if (sq != 2) return fail("x^(2^15) = x");
        uint32_t p = 1;
        for (unsigned n = 0; n < 2 * ph::kXOrder + 5; n++) {                                   // every exponent, and once more round
            if (ph::xpow(n) != p) return fail("xpow", (long)n);
            p = mul_x(p);
        }
        if (ph::xpow(ph::kXOrder) != 1) return fail("x^32767 = 1");
        unsigned s = 99;
        for (int t = 0; t < 20000; t++) {
            s = s * 1664525u + 1013904223u; const uint32_t a = s >> 16;
            s = s * 1664525u + 1013904223u; const uint32_t b = s >> 16;
            if (ph::mulmod(a, b) != mul_bitwise(a, b)) return fail("mulmod", (long)a, (long)b);
            s = s * 1664525u + 1013904223u; const uint32_t bytes = s >> (t % 28);
            if (ph::shift_bytes(a, bytes, lo, hi) != mul_bitwise(a, ph::xpow(ph::mod_order(8u * ph::mod_order(bytes))))) return fail("shift_bytes", (long)bytes);
            if (ph::mod_order(s) != s % ph::kXOrder) return fail("mod_order", (long)s);
        }
        // shift_bytes(r, n) is what n zero bytes do to the direct form
        uint32_t r = 0xBEEF;
        for (uint32_t n = 0; n < 5000; n++) { if (ph::shift_bytes(0xBEEFu, n, lo, hi) != r) return fail("shift_bytes against zero bytes", (long)n); r = ph::crc_byte(r, 0); }
    }
    // surfaces: the sizes of tests/test_pichash_gpu.py and what lies around the 16-byte run and the 16-row band, tight and padded, random and constant
    static const int kSizes[][2] = {{2, 2}, {8, 8}, {24, 16}, {264, 8}, {8, 264}, {520, 520}, {66, 34}, {16, 16}, {18, 18}, {30, 14}, {32, 48}, {34, 50},
                                    {176, 144}, {200, 120}, {96, 80}, {1040, 6}};
    int walks = 0;
    for (auto &sz : kSizes) for (int pad : {0, 16, 6}) {
        if (walk(sz[0], sz[1], sz[0] + pad, 1234u + (unsigned)sz[0] * 31u + (unsigned)pad, -1, lo, hi, walks)) return 1;
        if (pad == 0) { if (walk(sz[0], sz[1], sz[0], 0, 0x00, lo, hi, walks) || walk(sz[0], sz[1], sz[0], 0, 0xFF, lo, hi, walks)) return 1; }
    }
    printf("ok: %d walks over %d sizes\n", walks, (int)(sizeof kSizes / sizeof kSizes[0]));
    return 0;
}
