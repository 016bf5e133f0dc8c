// jmcodec_amd/csrc/deint_packed.h -- the deinterlacer D of INTEGRATION.md "Deinterlaced output" on 16-byte column chunks (k_deint, out_kernels.hip).
//
// D keeps the rows of one parity and rebuilds the others, plane by plane: mode 1 (bob) writes the rounded average i of the kept rows above and below,
// mode 2 (comb-adaptive) writes i only where the woven sample is combed, M = s[x-1] + 2 s[x] + s[x+1] > 4 T^2 with s = (up - cur) * (dn - cur).
// A lane owns one 16-byte chunk of a plane row and walks a strip of kDeintStrip rows: every row of the strip (and the one kept row just above it) is
// loaded once into registers, every row is stored once.  Per chunk and missing row:
//   * i of four samples: ONE v_lerp_u8;
//   * s: per sample two subtractions and one 24-bit multiply; it is kept NEGATED (ns = (up - cur) * (cur - dn)) so that the decision is the sign of
//     t = 4 T^2 + ns[x-1] + 2 ns[x] + ns[x+1] (v_mad_i32_i24, v_add3_u32): |t| < 2^24, so the TOP BYTE of t is 0xFF where the sample is combed and 0
//     elsewhere -- three v_perm_b32 gather four of them into a byte mask and one bit-select (v_bfi_b32; v_bitop3_b32 on gfx950) picks i or the woven sample for four samples;
//   * the horizontal neighbours across the chunk's edges come from two extra samples per side and row ("edge word"); at the plane's edges they repeat
//     the edge sample (cx clamps).  In the NV12 chroma plane the neighbour of a sample is two bytes away (STEP = 2).
// Everything is __host__ __device__: on the host the GPU instructions are restated in plain C++ (v_lerp_u8 / v_perm_b32 in mc_packed.h, the bit-select here),
// so tests/test_deinterlace_host.py runs the very strip routine of the kernel against a numpy restatement of D without a GPU
// (tests/native/deint_packed_check.cpp).
//
// The reference asks its decoder for cudaVideoDeinterlaceMode_Adaptive (nv_dec/nv_dec.cpp:508); what that does is not documented, D is
// this library's own definition.
#pragma once
#include "mc_packed.h"
#include <string.h>

namespace jmamd {
namespace dei {

#if defined(__HIP_DEVICE_COMPILE__)
#define JM_DEI_G __attribute__((address_space(1)))      // planes are global memory: global_load / global_store instead of flat ones
#define JM_DEI_UNROLL _Pragma("unroll")
#define JM_DEI_ROLLED _Pragma("nounroll")
#else
#define JM_DEI_G
#define JM_DEI_UNROLL
#define JM_DEI_ROLLED
#endif
typedef JM_DEI_G uint8_t gbyte;

constexpr int kDeintStrip = 8;          // rows a lane walks (even: a strip starts on a top-field row)

JM_HD uint32_t bfi(uint32_t mask, uint32_t a, uint32_t b) { return (a & mask) | (b & ~mask); }     // mask bit set -> a, else b (the compiler's pattern for v_bfi_b32 / v_bitop3_b32)

struct Chunk { uint32_t w[4]; };        // 16 samples of a row, sample k in byte k & 3 of w[k >> 2]

// sample q of the chunk, q in [-STEP, 16 + STEP): outside [0, 16) it comes from the edge word e (bytes 0 / 1: samples -2 / -1, bytes 2 / 3: 16 / 17)
JM_HD int sample_at(const Chunk &r, uint32_t e, int q) {
    return (int)(q < 0 ? (e >> (8 * (2 + q))) & 255u : (q >= 16 ? (e >> (8 * (q - 14))) & 255u : (r.w[q >> 2] >> (8 * (q & 3))) & 255u));
}

// mode 1: the rounded average of the kept rows above and below
JM_HD Chunk bob16(const Chunk &up, const Chunk &dn) {
    Chunk o;
    for (int k = 0; k < 4; k++) o.w[k] = pk::lerp(up.w[k], dn.w[k], pk::kOnes);
    return o;
}

// mode 2: up / cur / dn with their edge words, thr = 4 T^2
template <int STEP> JM_HD Chunk comb16(const Chunk &up, const Chunk &cur, const Chunk &dn, uint32_t eu, uint32_t ec, uint32_t ed, int thr) {
    int ns[16 + 2 * STEP];
    JM_DEI_UNROLL
    for (int q = -STEP; q < 16 + STEP; q++) {
        const int a = sample_at(up, eu, q), b = sample_at(cur, ec, q), c = sample_at(dn, ed, q);
        ns[q + STEP] = (a - b) * (b - c);                                   // -s: |ns| <= 65025
    }
    Chunk o;
    JM_DEI_UNROLL
    for (int k = 0; k < 4; k++) {
        uint32_t t[4];
        for (int j = 0; j < 4; j++) { const int x = 4 * k + j + STEP; t[j] = (uint32_t)(thr + ns[x - STEP] + ns[x + STEP] + 2 * ns[x]); }    // < 0: combed
        const uint32_t m01 = pk::perm(t[1], t[0], 0x0c0c0703u), m23 = pk::perm(t[3], t[2], 0x0c0c0703u);     // the top bytes (0xFF / 0x00) of t0 t1 | t2 t3
        const uint32_t mask = pk::perm(m23, m01, 0x05040100u);
        o.w[k] = bfi(mask, pk::lerp(up.w[k], dn.w[k], pk::kOnes), cur.w[k]);
    }
    return o;
}

// the n valid samples (bytes) at row[x ..], n <= 16 and a multiple of STEP; samples past the plane's right edge repeat the last one of their channel
// (cx clamps).  FAST: the row is 16-byte aligned and n == 16 -- one 16-byte load (and 16-byte / two 8-byte stores in store16).
template <int STEP, bool FAST> JM_HD Chunk load16(const gbyte *row, int x, int n) {
    Chunk c;
    if (FAST) {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        const u4 v = *(const JM_DEI_G u4 *)(row + x);
        c.w[0] = v.x; c.w[1] = v.y; c.w[2] = v.z; c.w[3] = v.w;
#else
        memcpy(c.w, row + x, 16);
#endif
        return c;
    }
    JM_DEI_UNROLL
    for (int k = 0; k < 4; k++) {
        uint32_t w = 0;
        JM_DEI_UNROLL
        for (int j = 0; j < 4; j++) { const int q = 4 * k + j, i = q < n ? q : n - STEP + ((q - n) & (STEP - 1)); w |= (uint32_t)row[x + i] << (8 * j); }
        c.w[k] = w;
    }
    return c;
}
// the edge word of the chunk c = load16(row, x, ...) of a plane row of W bytes: the samples left of x and right of x + 15, the chunk's own where there are none
template <int STEP, bool FAST> JM_HD uint32_t edge16(const gbyte *row, int x, int W, const Chunk &c) {
    uint32_t l, r;
    if (x > 0) l = FAST ? (uint32_t)*(const JM_DEI_G uint16_t *)(row + x - 2) : (uint32_t)row[x - 2] | (uint32_t)row[x - 1] << 8;
    else l = STEP == 1 ? (c.w[0] & 255u) << 8 : c.w[0] & 0xffffu;
    if (x + 16 < W) r = STEP == 1 ? (uint32_t)row[x + 16] : (FAST ? (uint32_t)*(const JM_DEI_G uint16_t *)(row + x + 16) : (uint32_t)row[x + 16] | (uint32_t)row[x + 17] << 8);
    else r = STEP == 1 ? c.w[3] >> 24 : c.w[3] >> 16;
    return l | r << 16;
}

// where the rows of one plane go: NV12-style rows of `pitch` bytes (d1 unused), or -- split -- the U and V planes of an I420 frame, rows of pitch bytes each
struct PlaneOut { gbyte *d0, *d1; int pitch; bool split; };

template <bool FAST> JM_HD void store16(const PlaneOut &o, int y, int x, int n, const Chunk &c) {
    if (!o.split) {
        gbyte *d = o.d0 + (size_t)y * o.pitch + x;
        if (FAST) {
#if defined(__HIP_DEVICE_COMPILE__)
            typedef uint32_t u4 __attribute__((ext_vector_type(4)));
            u4 v; v.x = c.w[0]; v.y = c.w[1]; v.z = c.w[2]; v.w = c.w[3];
            *(JM_DEI_G u4 *)d = v;
#else
            memcpy(d, c.w, 16);
#endif
        } else {
            JM_DEI_UNROLL
            for (int k = 0; k < 16; k++) if (k < n) d[k] = (uint8_t)(c.w[k >> 2] >> (8 * (k & 3)));        // (constant indices: the chunk stays in registers)
        }
        return;
    }
    gbyte *du = o.d0 + (size_t)y * o.pitch + (x >> 1), *dv = o.d1 + (size_t)y * o.pitch + (x >> 1);
    if (FAST) {
        // bytes 0 2 4 6 (U) / 1 3 5 7 (V) of a dword pair
        const uint32_t u0 = pk::perm(c.w[1], c.w[0], 0x06040200u), u1 = pk::perm(c.w[3], c.w[2], 0x06040200u);
        const uint32_t v0 = pk::perm(c.w[1], c.w[0], 0x07050301u), v1 = pk::perm(c.w[3], c.w[2], 0x07050301u);
#if defined(__HIP_DEVICE_COMPILE__)
        typedef uint32_t u2 __attribute__((ext_vector_type(2)));
        u2 a, b; a.x = u0; a.y = u1; b.x = v0; b.y = v1;
        *(JM_DEI_G u2 *)du = a; *(JM_DEI_G u2 *)dv = b;
#else
        memcpy(du, &u0, 4); memcpy(du + 4, &u1, 4); memcpy(dv, &v0, 4); memcpy(dv + 4, &v1, 4);
#endif
    } else {
        JM_DEI_UNROLL
        for (int k = 0; k < 8; k++) if (2 * k < n) { du[k] = (uint8_t)(c.w[k >> 1] >> (16 * (k & 1))); dv[k] = (uint8_t)(c.w[k >> 1] >> (16 * (k & 1) + 8)); }
    }
}

// One lane's work: one strip of the chunk at byte x of a plane of H rows (H >= 2) and W bytes per row (W even), source rows `pitch` bytes apart.
// Strip k of a plane whose rows of parity p are kept covers rows r0 .. r0 + 7 with r0 = 8 k + p - 1, so that in EVERY strip the rows at even offsets
// are the missing ones and those at odd offsets (and the row r0 - 1 just above the strip) are kept: one code path serves both parities, and the window
// -- slot j holds row r0 + j, j = -1 .. 7 -- lives in registers.  A plane has strip_count(H) strips (rows outside the plane are skipped).  The row above
// the plane is row 1 and the row below it row H - 2 (up() / dn() of the definition), so a missing row's neighbours are always slots j - 1 and j + 1.
// Only slots that are read are loaded (bob never reads a missing row).  COMB: mode 2 (else mode 1), thr = 4 T^2.  STEP 1: luma, 2: interleaved chroma.
JM_HD int strip_count(int H) { return H / kDeintStrip + 1; }
JM_HD int strip_row0(int k, int p) { return k * kDeintStrip + p - 1; }
JM_HD int window_row(int y, int H) { return y < 0 ? 1 : (y >= H ? H - 2 : y); }

// a whole chunk of aligned rows (source and destination): 16-byte loads, all of them before the first store, 16-byte stores
template <int STEP, bool COMB> JM_HD void deint_strip_fast(const gbyte *plane, int pitch, int W, int H, int x, int r0, int thr, const PlaneOut &out) {
    Chunk win[kDeintStrip + 1]; uint32_t edge[kDeintStrip + 1];
    JM_DEI_UNROLL
    for (int j = -1; j < kDeintStrip; j++) {
        if (!COMB && !(j & 1)) continue;
        const gbyte *row = plane + (size_t)window_row(r0 + j, H) * pitch;
        win[j + 1] = load16<STEP, true>(row, x, 16);
        if (COMB) edge[j + 1] = edge16<STEP, true>(row, x, W, win[j + 1]);
    }
    JM_DEI_UNROLL
    for (int j = 0; j < kDeintStrip; j++) {
        const int y = r0 + j;
        if (y < 0 || y >= H) continue;
        if (j & 1) store16<true>(out, y, x, 16, win[j + 1]);
        else if (!COMB) store16<true>(out, y, x, 16, bob16(win[j], win[j + 2]));
        else store16<true>(out, y, x, 16, comb16<STEP>(win[j], win[j + 1], win[j + 2], edge[j], edge[j + 1], edge[j + 2], thr));
    }
}
// any chunk (the last one of a row whose length is not a multiple of 16, rows that are not aligned): byte loads and stores, row by row
template <int STEP> JM_HD void deint_strip_slow(const gbyte *plane, int pitch, int W, int H, int x, int r0, int mode, int thr, const PlaneOut &out) {
    const int n = W - x < 16 ? W - x : 16;
    JM_DEI_ROLLED
    for (int j = 0; j < kDeintStrip; j++) {
        const int y = r0 + j;
        if (y < 0 || y >= H) continue;
        const gbyte *row = plane + (size_t)y * pitch, *ru = plane + (size_t)window_row(y - 1, H) * pitch, *rd = plane + (size_t)window_row(y + 1, H) * pitch;
        if (j & 1) { store16<false>(out, y, x, n, load16<STEP, false>(row, x, n)); continue; }
        const Chunk up = load16<STEP, false>(ru, x, n), dn = load16<STEP, false>(rd, x, n);
        if (mode != 2) { store16<false>(out, y, x, n, bob16(up, dn)); continue; }
        const Chunk cur = load16<STEP, false>(row, x, n);
        store16<false>(out, y, x, n, comb16<STEP>(up, cur, dn, edge16<STEP, false>(ru, x, W, up), edge16<STEP, false>(row, x, W, cur),
            edge16<STEP, false>(rd, x, W, dn), thr));
    }
}
// strip k of the chunk at x: mode 1 / 2, p = parity of the kept rows
template <int STEP> JM_HD void deint_strip(const gbyte *plane, int pitch, int W, int H, int x, int k, int mode, int p, int thr, const PlaneOut &out) {
    const int r0 = strip_row0(k, p);
    // (16-byte rows on both sides; the two planes of a split destination take 8 bytes of a chunk each)
    const bool aligned = (((uintptr_t)plane | (uintptr_t)pitch) & 15) == 0 &&
        (out.split ? ((uintptr_t)out.d0 | (uintptr_t)out.d1 | (uintptr_t)out.pitch) & 7 : ((uintptr_t)out.d0 | (uintptr_t)out.pitch) & 15) == 0;
    if (W - x >= 16 && aligned) {
        if (mode == 2) deint_strip_fast<STEP, true>(plane, pitch, W, H, x, r0, thr, out);
        else deint_strip_fast<STEP, false>(plane, pitch, W, H, x, r0, thr, out);
    } else deint_strip_slow<STEP>(plane, pitch, W, H, x, r0, mode, thr, out);
}

// A whole frame as k_deint sees it: work item i of frame_items(w, h) -- the luma strips row-major (chunk fastest), then the strips of the interleaved
// chroma plane.  Source: a pitch-linear NV12 surface (chroma rows from byte chroma_offset); destination: NV12 at dst_pitch / dst_chroma_offset
// (out_fmt 0) or a tight I420 frame (out_fmt 1).
JM_HD int frame_items(int w, int h) { return ((w + 15) >> 4) * (strip_count(h) + strip_count(h >> 1)); }
JM_HD void deint_item(const gbyte *src, gbyte *dst, int pitch, int chroma_offset, int w, int h, int dst_pitch, int dst_chroma_offset, int out_fmt, int mode,
                      int parity, int thr, int i) {
    const int h2 = h >> 1, cpr = (w + 15) >> 4, nl = cpr * strip_count(h);
    const bool chroma = i >= nl;
    const int j = chroma ? i - nl : i, x = (j % cpr) * 16, k = j / cpr;
    if (!chroma) deint_strip<1>(src, pitch, w, h, x, k, mode, parity, thr, PlaneOut{dst, nullptr, out_fmt == 0 ? dst_pitch : w, false});
    else if (out_fmt == 0) deint_strip<2>(src + chroma_offset, pitch, w, h2, x, k, mode, parity, thr, PlaneOut{dst + dst_chroma_offset, nullptr, dst_pitch, false});
    else { gbyte *u = dst + (size_t)w * h;
        deint_strip<2>(src + chroma_offset, pitch, w, h2, x, k, mode, parity, thr, PlaneOut{u, u + (size_t)(w >> 1) * h2, w >> 1, true}); }
}

}  // namespace dei
}  // namespace jmamd
