// jmcodec_amd/csrc/md5_packed.h -- the per-lane routines of k_hevc_md5 (pichash.hip): the MD5 (RFC 1321) of the decoded picture hash SEI (H.265
// D.3.19, hash_type 0) of one colour component.  INTEGRATION.md "Picture hash" defines it: the component's samples as a raster byte array of the coded
// size (Y: w h bytes; Cb, Cr: (w / 2) (h / 2) bytes each, de-interleaved from the NV12 surface), one byte per sample.
//
// MD5 is one serial chain per component: 64 steps per 64-byte block, each waiting for the one before it.  Nothing in it can be spread over lanes, so
// the kernel splits the WORK AROUND the chain instead.  The component's byte stream -- samples, then the RFC's padding (0x80, zeros, the bit length as
// 64 bits little-endian) up to whole blocks -- is cut into tiles of kMd5TileBytes.  Three routines:
//   sample_offset   stream byte -> surface byte (rows gathered at `pitch`, chroma de-interleaved);
//   stage_item      16 bytes of the padded stream as four little-endian words: what a staging lane puts into the LDS tile.  One 16-byte load (two
//                   for chroma, split by v_perm_b32) when the run lies in one row and is aligned, byte loads of exactly the samples otherwise;
//   block           the 64 steps over one block of 16 words.  Per step on the device: one v_bitop3_b32 (the round function), one v_add3_u32,
//                   one v_alignbit_b32 (the rotate), one v_add_u32; M[g] + K[i] does not depend on the chain.
// Every function is __host__ __device__ (mc_packed.h): tools/md5_asan.cpp plays the kernel on the CPU with them, against the RFC's test suite and
// hashlib.  On the host the rotate and the bit functions are restated in plain C++.
#pragma once
#include <stddef.h>
#include "pichash_packed.h"       // ph::sbyte / ph::suint4 (global address space on the device), pk::perm

namespace jmamd {
namespace md5 {

constexpr int kMd5TileBytes = 4096;                    // bytes of the padded stream per LDS tile and workgroup barrier; a multiple of 64
constexpr int kTileWords = kMd5TileBytes / 4;
static_assert(kMd5TileBytes % 64 == 0 && kMd5TileBytes >= 128, "a tile holds whole blocks");

constexpr uint32_t kInit[4] = {0x67452301u, 0xEFCDAB89u, 0x98BADCFEu, 0x10325476u};
constexpr uint32_t kK[64] = {                          // floor(2^32 |sin(i + 1)|)
    0xD76AA478u, 0xE8C7B756u, 0x242070DBu, 0xC1BDCEEEu, 0xF57C0FAFu, 0x4787C62Au, 0xA8304613u, 0xFD469501u,
    0x698098D8u, 0x8B44F7AFu, 0xFFFF5BB1u, 0x895CD7BEu, 0x6B901122u, 0xFD987193u, 0xA679438Eu, 0x49B40821u,
    0xF61E2562u, 0xC040B340u, 0x265E5A51u, 0xE9B6C7AAu, 0xD62F105Du, 0x02441453u, 0xD8A1E681u, 0xE7D3FBC8u,
    0x21E1CDE6u, 0xC33707D6u, 0xF4D50D87u, 0x455A14EDu, 0xA9E3E905u, 0xFCEFA3F8u, 0x676F02D9u, 0x8D2A4C8Au,
    0xFFFA3942u, 0x8771F681u, 0x6D9D6122u, 0xFDE5380Cu, 0xA4BEEA44u, 0x4BDECFA9u, 0xF6BB4B60u, 0xBEBFBC70u,
    0x289B7EC6u, 0xEAA127FAu, 0xD4EF3085u, 0x04881D05u, 0xD9D4D039u, 0xE6DB99E5u, 0x1FA27CF8u, 0xC4AC5665u,
    0xF4292244u, 0x432AFF97u, 0xAB9423A7u, 0xFC93A039u, 0x655B59C3u, 0x8F0CCC92u, 0xFFEFF47Du, 0x85845DD1u,
    0x6FA87E4Fu, 0xFE2CE6E0u, 0xA3014314u, 0x4E0811A1u, 0xF7537E82u, 0xBD3AF235u, 0x2AD7D2BBu, 0xEB86D391u};
constexpr int kS[4][4] = {{7, 12, 17, 22}, {5, 9, 14, 20}, {4, 11, 16, 23}, {6, 10, 15, 21}};

#if defined(__HIP_DEVICE_COMPILE__)
JM_HD uint32_t rotl(uint32_t x, int s) { return __builtin_amdgcn_alignbit(x, x, (uint32_t)(32 - s)); }          // ({x, x} >> (32 - s)) & 0xFFFFFFFF
// v_bitop3_b32: bit k of the result is bit (4 x[k] + 2 y[k] + z[k]) of the table
JM_HD uint32_t fF(uint32_t x, uint32_t y, uint32_t z) { return __builtin_amdgcn_bitop3_b32(x, y, z, 0xCA); }
JM_HD uint32_t fG(uint32_t x, uint32_t y, uint32_t z) { return __builtin_amdgcn_bitop3_b32(x, y, z, 0xE4); }
JM_HD uint32_t fH(uint32_t x, uint32_t y, uint32_t z) { return __builtin_amdgcn_bitop3_b32(x, y, z, 0x96); }
JM_HD uint32_t fI(uint32_t x, uint32_t y, uint32_t z) { return __builtin_amdgcn_bitop3_b32(x, y, z, 0x39); }
#else
// ---- the same two instructions in plain C++ (RFC 1321 section 3.4) ----
JM_HD uint32_t rotl(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }
JM_HD uint32_t fF(uint32_t x, uint32_t y, uint32_t z) { return (x & y) | (~x & z); }
JM_HD uint32_t fG(uint32_t x, uint32_t y, uint32_t z) { return (x & z) | (y & ~z); }
JM_HD uint32_t fH(uint32_t x, uint32_t y, uint32_t z) { return x ^ y ^ z; }
JM_HD uint32_t fI(uint32_t x, uint32_t y, uint32_t z) { return y ^ (x | ~z); }
#endif

// one 64-byte block (16 little-endian words) through the chain
JM_HD void block(uint32_t *state, const uint32_t *m) {
    uint32_t a = state[0], b = state[1], c = state[2], d = state[3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 64; i++) {
        const int r = i >> 4;
        const int g = r == 0 ? i : (r == 1 ? (5 * i + 1) & 15 : (r == 2 ? (3 * i + 5) & 15 : (7 * i) & 15));
        const uint32_t f = r == 0 ? fF(b, c, d) : (r == 1 ? fG(b, c, d) : (r == 2 ? fH(b, c, d) : fI(b, c, d)));
        const uint32_t mk = m[g] + kK[i];                         // (off the chain)
        const uint32_t t = a + f + mk;
        a = d; d = c; c = b; b = b + rotl(t, kS[r][i & 3]);
    }
    state[0] += a; state[1] += b; state[2] += c; state[3] += d;
}

// ---- the component's byte stream -----------------------------------------------------------------------------------------------------------------
JM_HD uint32_t comp_bytes(int w, int h, int c) { return c == 0 ? (uint32_t)w * (uint32_t)h : (uint32_t)(w >> 1) * (uint32_t)(h >> 1); }
// the stream of n bytes with its padding: 0x80, zeros, eight length bytes, up to whole blocks
JM_HD uint32_t padded_bytes(uint32_t n) { return ((n + 8u) / 64u + 1u) * 64u; }
JM_HD int tile_count(uint32_t n) { return (int)((padded_bytes(n) + (uint32_t)kMd5TileBytes - 1u) / (uint32_t)kMd5TileBytes); }
JM_HD int tile_blocks(uint32_t n, int t) {
    const uint32_t rest = padded_bytes(n) - (uint32_t)t * (uint32_t)kMd5TileBytes;
    return (int)((rest < (uint32_t)kMd5TileBytes ? rest : (uint32_t)kMd5TileBytes) / 64u);
}
JM_HD int tile_items(uint32_t n, int t) { return 4 * tile_blocks(n, t); }          // 16 bytes each
// where sample (x, row) of component c (0 Y, 1 Cb, 2 Cr) lies in the NV12 surface
JM_HD size_t surface_offset(int c, uint32_t row, uint32_t x, int pitch, int chroma_offset) {
    return c == 0 ? (size_t)row * (size_t)pitch + x : (size_t)chroma_offset + (size_t)row * (size_t)pitch + 2u * x + (uint32_t)(c - 1);
}
// ... and stream byte q (below the component's byte count)
JM_HD size_t sample_offset(int c, uint32_t q, int w, int pitch, int chroma_offset) {
    const uint32_t cw = (uint32_t)(c == 0 ? w : w >> 1), row = q / cw;
    return surface_offset(c, row, q - row * cw, pitch, chroma_offset);
}
// byte q >= n of the padded stream
JM_HD uint32_t pad_byte(uint32_t q, uint32_t n) {
    const uint32_t len_at = padded_bytes(n) - 8u;
    if (q == n) return 0x80u;
    if (q < len_at) return 0u;
    return (uint32_t)((((uint64_t)n << 3) >> (8u * (q - len_at))) & 255u);
}

// ---- one staging item of k_hevc_md5, shared with the CPU walk -------------------------------------------------------------------------------------
// Item i of tile t of component c: bytes t * kMd5TileBytes + 16 i .. + 15 of the padded stream, as four little-endian words (the tile's words
// 4 i .. 4 i + 3).  wide: the surface's address, pitch and chroma offset are multiples of 16 -- a run of 16 samples inside one row whose first byte is
// aligned is one 16-byte load (chroma: two, of the 32 bytes that hold the 16 Cb Cr pairs); everything else -- a run that crosses a row end, an
// unaligned one, the padding -- goes byte by byte and reads exactly the samples.
JM_HD void stage_item(const ph::sbyte *surf, int pitch, int chroma_offset, int w, int h, int c, int t, int i, bool wide, uint32_t *out) {
    const uint32_t n = comp_bytes(w, h, c), s = (uint32_t)t * (uint32_t)kMd5TileBytes + 16u * (uint32_t)i;
    const uint32_t cw = (uint32_t)(c == 0 ? w : w >> 1);
    uint32_t row = s / cw, x = s - row * cw;
    out[0] = out[1] = out[2] = out[3] = 0u;
    const uint32_t xb = c == 0 ? x : 2u * x;
    if (wide && s + 16u <= n && x + 16u <= cw && (xb & 15u) == 0u) {
        const ph::sbyte *p = surf + (c == 0 ? (size_t)0 : (size_t)chroma_offset) + (size_t)row * (size_t)pitch + xb;
        uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 v0 = *(const ph::suint4 *)p;
        d[0] = v0.x; d[1] = v0.y; d[2] = v0.z; d[3] = v0.w;
        if (c != 0) { const uint4 v1 = *(const ph::suint4 *)(p + 16); d[4] = v1.x; d[5] = v1.y; d[6] = v1.z; d[7] = v1.w; }
#else
        for (int j = 0; j < (c == 0 ? 16 : 32); j++) d[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
#endif
        if (c == 0) { out[0] = d[0]; out[1] = d[1]; out[2] = d[2]; out[3] = d[3]; }
        else {
            const uint32_t sel = c == 1 ? 0x06040200u : 0x07050301u;      // the even (Cb) or the odd (Cr) bytes of eight
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int k = 0; k < 4; k++) out[k] = pk::perm(d[2 * k + 1], d[2 * k], sel);
        }
        return;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 16; j++) {
        const uint32_t q = s + (uint32_t)j;
        const uint32_t b = q < n ? (uint32_t)surf[surface_offset(c, row, x, pitch, chroma_offset)] : pad_byte(q, n);
        out[j >> 2] |= b << (8 * (j & 3));
        if (++x == cw) { x = 0; row++; }
    }
}

}  // namespace md5
}  // namespace jmamd
