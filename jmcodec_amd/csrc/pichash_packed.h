// jmcodec_amd/csrc/pichash_packed.h -- the per-lane arithmetic of k_hevc_pichash (pichash.hip): the two decoded-picture hashes of H.265 D.3.19 that can
// be computed in parallel, on PACKED bytes.  INTEGRATION.md "Picture hash" defines both exactly.
//
// checksum: sum over the component's samples of s[y][x] ^ m(x, y), m = (x & 255) ^ (y & 255) ^ (x >> 8) ^ (y >> 8), mod 2^32.  A lane owns a run of
//   4, 8 or 16 consecutive samples of one row that starts at a multiple of 16 (luma) or 8 (chroma): inside it m = c ^ j with one c per run, so a dword
//   is XORed with four mask bytes at once and its bytes are summed by one v_dot4_u32_u8.
// CRC: crc = 0xFFFF, 16 zero bits appended, MSB first, polynomial P = x^16 + x^12 + x^5 + 1 -- the same value as the "direct" form with initial value
//   0x1D0F and no appended bits (CRC-16/SPI-FUJITSU).  The direct form is linear over GF(2): with R(c) = the direct CRC of chunk c from initial value 0,
//       CRC(picture) = XOR_k R(chunk_k) * x^(8 * bytes behind chunk k)  ^  0x1D0F * x^(8 * bytes of the picture)        (mod P)
//   so every lane computes R of its own run with crc_byte and moves it to its place with one multiplication by a power of x.
// Powers of x: kXPow2[k] = x^(2^k) mod P; xpow(n) multiplies the entries of n's set bits (16-step carry-less products, mulmod).  P = (x + 1) * (a
//   primitive polynomial of degree 15), so x has order 2^15 - 1 = 32767 -- the table repeats after 15 entries, and an exponent of any size is first
//   reduced mod 32767 by folding its 15-bit digits (2^15 = 1 mod 32767): no division anywhere.  The kernel looks x^e, e < 32767, up as the product of
//   two small tables (fill_pow_tables) instead of walking 15 bits per lane.
// Every function is __host__ __device__ (mc_packed.h): tools/pichash_asan.cpp walks them on the CPU against a bit-serial CRC and the plain checksum loop.
#pragma once
#include <stddef.h>
#include "mc_packed.h"

namespace jmamd {
namespace ph {

// surface bytes: a global (address space 1) pointer on the device, so that the loads are global_load and not FLAT (deblock_device.h)
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(1))) uint8_t sbyte;
typedef __attribute__((address_space(1))) uint4 suint4;
#else
typedef uint8_t sbyte;
#endif

constexpr uint32_t kCrcInit = 0x1D0Fu;                 // 0xFFFF followed through 16 steps of the augmented form = the direct form's initial value
constexpr uint32_t kXOrder = 32767u;                   // x^32767 = 1 mod P
constexpr uint16_t kXPow2[15] = {0x0002, 0x0004, 0x0010, 0x0100, 0x1021, 0x3730, 0xB861, 0xAEFC, 0x8E29, 0x13FC, 0x36C4, 0xFD50, 0xAA9E, 0x881C, 0x4458};
constexpr int kPowLo = 256, kPowHi = 128;              // x^e = lo[e & 255] * hi[e >> 8]

// one byte through the direct form (the table-free step for this polynomial: the byte's reduction is three shifts of t ^ t >> 4)
JM_HD uint32_t crc_byte(uint32_t crc, uint32_t b) {
    uint32_t t = ((crc >> 8) ^ b) & 255u;
    t ^= t >> 4;
    return ((crc << 8) ^ (t << 12) ^ (t << 5) ^ t) & 0xFFFFu;
}
// a * b mod P, both below 2^16: the carry-less product (below 2^31), then its upper half times x^16 -- which is the direct CRC of those two bytes
JM_HD uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 16; i++) p ^= (0u - ((b >> i) & 1u)) & (a << i);
    return crc_byte(crc_byte(0u, p >> 24), (p >> 16) & 255u) ^ (p & 0xFFFFu);
}
JM_HD uint32_t mod_order(uint32_t n) {                 // n mod 32767
    n = (n & 0x7FFFu) + (n >> 15);                     // < 2^17 + 2^15
    n = (n & 0x7FFFu) + (n >> 15);                     // <= 32767 + 4
    n = (n & 0x7FFFu) + (n >> 15);                     // <= 32767
    return n == kXOrder ? 0u : n;
}
// the exponent of x that moves a chunk past `bytes` bytes
JM_HD uint32_t byte_exponent(uint32_t bytes) { return mod_order(8u * mod_order(bytes)); }
JM_HD uint32_t xpow(uint32_t n) {                      // x^n mod P, any n
    n = mod_order(n);
    uint32_t r = 1u;
    for (int k = 0; k < 15; k++) if ((n >> k) & 1u) r = mulmod(r, kXPow2[k]);
    return r;
}
// the kernel's two tables: lo[i] = x^i, hi[i] = x^(256 i)
JM_HD void fill_pow_tables(uint16_t *lo, uint16_t *hi) {
    for (int i = 0; i < kPowLo; i++) lo[i] = (uint16_t)xpow((uint32_t)i);
    for (int i = 0; i < kPowHi; i++) hi[i] = (uint16_t)xpow(256u * (uint32_t)i);
}
// r * x^(8 * bytes) through the tables
JM_HD uint32_t shift_bytes(uint32_t r, uint32_t bytes, const uint16_t *lo, const uint16_t *hi) {
    const uint32_t e = byte_exponent(bytes);
    return mulmod(mulmod(r, lo[e & 255u]), hi[e >> 8]);
}

// WORDS dwords (4, 8 or 16 bytes) of one component's row: the first n bytes are samples x0 .. x0 + n - 1 of row y, 4 * WORDS | x0.  Adds their checksum
// terms to sum and returns R of the n bytes.
template <int WORDS> JM_HD uint32_t hash_run(const uint32_t *w, int n, int x0, int y, uint32_t &sum) {
    const uint32_t c = (uint32_t)((x0 & 255) ^ (y & 255) ^ (x0 >> 8) ^ (y >> 8));     // m of the run's first sample; sample j: c ^ j
    uint32_t crc = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < WORDS; k++) {
        const int nv = n - 4 * k;                                                    // samples of this dword
        if (nv <= 0) continue;
        const uint32_t keep = nv >= 4 ? 0xFFFFFFFFu : (1u << (8 * nv)) - 1u;
        const uint32_t m = (c * 0x01010101u) ^ (0x03020100u + 0x04040404u * (uint32_t)k);
        sum = pk::udot4((w[k] ^ m) & keep, 0x01010101u, sum);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 4; j++) if (j < nv) crc = crc_byte(crc, (w[k] >> (8 * j)) & 255u);
    }
    return crc;
}
// Cb (even bytes) or Cr (odd bytes) of 2 * HALF dwords of an NV12 chroma row, as HALF dwords of one component
template <int HALF> JM_HD void split_uv(const uint32_t *uv, uint32_t *cb, uint32_t *cr) {
    for (int k = 0; k < HALF; k++) { cb[k] = pk::perm(uv[2 * k + 1], uv[2 * k], 0x06040200u); cr[k] = pk::perm(uv[2 * k + 1], uv[2 * k], 0x07050301u); }
}

// ---- one work item of k_hevc_pichash, shared with the CPU walk ----------------------------------------------------------------------------------
// A surface row (w bytes: luma samples, or Cb Cr pairs) is cut into 16-byte runs; item i of band `band` (kBandRows luma rows and the chroma rows below
// them) is run i % runs of row i / runs, the band's luma rows first, then its chroma rows.
constexpr int kBandRows = 16;
struct Acc { uint32_t sum_y = 0, sum_cb = 0, sum_cr = 0, crc_y = 0, crc_cb = 0, crc_cr = 0; };      // (scalars: an indexed member would live in scratch)
JM_HD int band_count(int h) { return (h + kBandRows - 1) / kBandRows; }
JM_HD int band_items(int w, int h, int band) {
    const int rows = h - band * kBandRows < kBandRows ? h - band * kBandRows : kBandRows;
    return ((w + 15) >> 4) * (rows + (rows >> 1));
}
// wide: the surface's address, pitch and chroma offset are multiples of 16 -- a whole run is one 16-byte load; else, and for a row's last partial
// run, byte loads of exactly the n samples
JM_HD void hash_item(const sbyte *surf, int pitch, int chroma_offset, int w, int h, int band, int i, bool wide, const uint16_t *lo, const uint16_t *hi,
                     Acc &a) {
    const int runs = (w + 15) >> 4, y0 = band * kBandRows, rows = h - y0 < kBandRows ? h - y0 : kBandRows;
    const int r = i / runs, x0 = 16 * (i - r * runs), n = w - x0 < 16 ? w - x0 : 16;
    const bool chroma = r >= rows;
    const int y = chroma ? (y0 >> 1) + (r - rows) : y0 + r;
    const sbyte *p = surf + (chroma ? (size_t)chroma_offset : 0) + (size_t)y * pitch + x0;
    uint32_t d[4] = {0, 0, 0, 0};
    if (wide && n == 16) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 v = *(const suint4 *)p;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
#else
        for (int j = 0; j < 16; j++) d[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
#endif
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 16; j++) if (j < n) d[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    }
    // (every accumulator is updated on both paths: an update of one OR the other is compiled into a store through a selected address, i.e. scratch)
    uint32_t s0 = 0, s1 = 0, s2 = 0, c0 = 0, c1 = 0, c2 = 0;
    if (!chroma) {
        const uint32_t behind = (uint32_t)(h - 1 - y) * (uint32_t)w + (uint32_t)(w - x0 - n);
        c0 = shift_bytes(hash_run<4>(d, n, x0, y, s0), behind, lo, hi);
    } else {
        uint32_t cb[2], cr[2];
        split_uv<2>(d, cb, cr);
        const int cw = w >> 1, ch = h >> 1, xc = x0 >> 1, nc = n >> 1;
        const uint32_t behind = (uint32_t)(ch - 1 - y) * (uint32_t)cw + (uint32_t)(cw - xc - nc);
        c1 = shift_bytes(hash_run<2>(cb, nc, xc, y, s1), behind, lo, hi);
        c2 = shift_bytes(hash_run<2>(cr, nc, xc, y, s2), behind, lo, hi);
    }
    a.sum_y += s0; a.sum_cb += s1; a.sum_cr += s2; a.crc_y ^= c0; a.crc_cb ^= c1; a.crc_cr ^= c2;
}
// the term of the initial value: once per component
JM_HD uint32_t init_term(uint32_t bytes, const uint16_t *lo, const uint16_t *hi) { return shift_bytes(kCrcInit, bytes, lo, hi); }

}  // namespace ph
}  // namespace jmamd
