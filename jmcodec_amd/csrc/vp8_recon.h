// jmcodec_amd/csrc/vp8_recon.h -- the sample arithmetic of VP8 decode (codec_type 5), INTEGRATION.md "VP8": dequantisation, the inverse
// Walsh-Hadamard transform and the inverse DCT of RFC 6386 section 14, the intra prediction of section 12, the loop filters of section 15 and (option
// vp8_inter; k_vp8_inter, tests/native/vp8_inter_check.cpp, tools/vp8_inter_asan.cpp) the inter prediction of section 18, as
// __host__ __device__ LANE routines: each takes the lane number and does that lane's share of one macroblock, on a small work area (LDS in the
// kernels, plain memory on the host).  k_vp8_recon / k_vp8_filter (vp8_kernels.hip) call them with threadIdx; tests/native/vp8_check.cpp,
// tools/vp8_asan.cpp and tools/fuzz_vp8.cpp call them for lane 0..63 in turn, phase after phase, macroblocks in the kernels' wavefront order -- so the
// CPU checks run the kernels' own arithmetic and addressing.  Between two phases the kernels place a wave-level barrier; within a phase no lane
// reads what another lane writes.  All int32 with arithmetic >>; the transforms' products are exact (|coefficient| < 2^15, constants < 2^16).
#pragma once
#include "jpeg_recon.h"     // JR_HD, JR_UNROLL, jpeg_clip
#include "vp8_jobs.h"
#include <stddef.h>
#include <string.h>

namespace jmamd {

// ---- the reconstruction work area of one macroblock --------------------------------------------------------------------------------------------
// y: 17 rows of kVp8YS bytes.  Row 0 is the row above the macroblock, rows 1..16 the macroblock; column 3 is the column to its left (row 0: the
// corner), columns 4..19 the macroblock, columns 20..23 the four above-right samples -- in row 0, and repeated in rows 4, 8 and 12, where the
// sub-blocks of column 3 in sub-block rows 1..3 look for them (they come from the row above the macroblock: RFC 6386 12.3).
// u, v: 9 rows of kVp8CS bytes, the same layout without above-right samples.
constexpr int kVp8YS = 24, kVp8CS = 12;
struct Vp8Work {
    int16_t coef[25][16];          // dequantised coefficients, raster order inside a block; block 24 = Y2
    int16_t pad[8];
    int res[24][16];               // residuals
    uint8_t y[17 * kVp8YS];
    uint8_t u[9 * kVp8CS + 4], v[9 * kVp8CS + 4];
};
constexpr int kVp8CoefDwords = (25 * 16 + 8) / 2;

JR_HD uint8_t vp8_clamp255(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

JR_HD void vp8_zero_lane(Vp8Work &w, int lane) {
    uint32_t *p = reinterpret_cast<uint32_t *>(&w.coef[0][0]);
    for (int i = lane; i < kVp8CoefDwords; i += 64) p[i] = 0;
}

// the macroblock's entries into coef[], dequantised.  Bounded by the record's count (at most kVp8MaxMbEntries), by n_entries and by the block number
JR_HD void vp8_scatter_lane(Vp8Work &w, const Vp8Mb &mb, const uint32_t *entries, int n_entries, const int16_t *dq, int lane) {
    const int cnt = mb.count < kVp8MaxMbEntries ? mb.count : kVp8MaxMbEntries;
    for (int e = lane; e < cnt; e += 64) {
        const uint32_t idx = mb.first + (uint32_t)e;
        if (idx >= (uint32_t)n_entries || idx < mb.first) break;
        const uint32_t v = entries[idx];
        const int pos = (int)(v & 15), blk = (int)(v >> 4 & 31);
        if (blk > 24) continue;
        const int t = blk == 24 ? 2 : (blk >= 16 ? 4 : 0);
        w.coef[blk][pos] = (int16_t)((int)(int16_t)(v >> 16) * dq[t + (pos ? 1 : 0)]);
    }
}

// RFC 6386 14.3, the inverse WHT: output idx (= luma block idx) of the Y2 block `in` (exact for a lone DC too: every output is (in[0] + 3) >> 3)
JR_HD int vp8_iwht_at(const int16_t *in, int idx) {
    const int i = idx >> 2, k = idx & 3;
    int t[4];
JR_UNROLL
    for (int j = 0; j < 4; j++) {
        const int a1 = in[j] + in[12 + j], b1 = in[4 + j] + in[8 + j], c1 = in[4 + j] - in[8 + j], d1 = in[j] - in[12 + j];
        t[j] = i == 0 ? a1 + b1 : (i == 1 ? c1 + d1 : (i == 2 ? a1 - b1 : d1 - c1));
    }
    const int a1 = t[0] + t[3], b1 = t[1] + t[2], c1 = t[1] - t[2], d1 = t[0] - t[3];
    const int o = k == 0 ? a1 + b1 : (k == 1 ? c1 + d1 : (k == 2 ? a1 - b1 : d1 - c1));
    return (int16_t)((o + 3) >> 3);
}
// lanes 0..15: the DC of luma block `lane` of a macroblock with a Y2 block
JR_HD void vp8_wht_lane(Vp8Work &w, int lane) { if (lane < 16) w.coef[lane][0] = (int16_t)vp8_iwht_at(w.coef[24], lane); }

// RFC 6386 14.3, the inverse DCT: columns first, then rows with (x + 4) >> 3
JR_HD void vp8_idct(const int16_t *c, int *r) {
    int t[16];
JR_UNROLL
    for (int i = 0; i < 4; i++) {
        const int c0 = c[i], c1 = c[4 + i], c2 = c[8 + i], c3 = c[12 + i];
        const int a1 = c0 + c2, b1 = c0 - c2;
        const int cc = ((c1 * 35468) >> 16) - (c3 + ((c3 * 20091) >> 16));
        const int d1 = (c1 + ((c1 * 20091) >> 16)) + ((c3 * 35468) >> 16);
        // (16-bit words between the passes, as in the RFC's procedure: with them no product below can leave int32, whatever the coefficients)
        t[i] = (int16_t)(a1 + d1); t[4 + i] = (int16_t)(b1 + cc); t[8 + i] = (int16_t)(b1 - cc); t[12 + i] = (int16_t)(a1 - d1);
    }
JR_UNROLL
    for (int i = 0; i < 4; i++) {
        const int c0 = t[4 * i], c1 = t[4 * i + 1], c2 = t[4 * i + 2], c3 = t[4 * i + 3];
        const int a1 = c0 + c2, b1 = c0 - c2;
        const int cc = ((c1 * 35468) >> 16) - (c3 + ((c3 * 20091) >> 16));
        const int d1 = (c1 + ((c1 * 20091) >> 16)) + ((c3 * 35468) >> 16);
        r[4 * i] = (a1 + d1 + 4) >> 3; r[4 * i + 1] = (b1 + cc + 4) >> 3; r[4 * i + 2] = (b1 - cc + 4) >> 3; r[4 * i + 3] = (a1 - d1 + 4) >> 3;
    }
}
// lanes 0..23: the residual of block `lane` (a block without entries -- and, for luma with Y2, a zero DC -- is all zero and skips the arithmetic)
JR_HD void vp8_idct_lane(Vp8Work &w, const Vp8Mb &mb, int lane) {
    if (lane >= 24) return;
    const bool some = (mb.nz >> lane & 1) || (lane < 16 && mb.ymode != VP8_B_PRED && w.coef[lane][0] != 0);
    if (some) vp8_idct(w.coef[lane], w.res[lane]);
    else {
JR_UNROLL
        for (int i = 0; i < 16; i++) w.res[lane][i] = 0;
    }
}

// The samples around the macroblock into the work area: 127 above the frame, 129 to its left; the corner is 127 in macroblock row 0 and 129 in
// column 0 below it; the above-right samples of the last macroblock of a row (below row 0) repeat sample 15 of the row above (libwebp's rule, which
// tests/golden/vp8 pins).  83 elements: 21 above (corner, 16, 4 above right), 16 left, 3 x 4 copies of the above-right samples, 2 x (9 + 8) chroma.
// Reads: row 16 mby - 1, columns 16 mbx - 1 .. 16 mbx + 19 (the last four only when mbx < mb_w - 1), and column 16 mbx - 1 -- all inside the surface.
JR_HD void vp8_borders_lane(Vp8Work &w, const uint8_t *surf, int pitch, int chroma_offset, int mbx, int mby, int mb_w, int lane) {
    const uint8_t *Y = surf + (size_t)(mby * 16) * pitch + mbx * 16;
    const uint8_t *C = surf + chroma_offset + (size_t)(mby * 8) * pitch + mbx * 16;
    for (int i = lane; i < 83; i += 64) {
        if (i < 21 || (i >= 37 && i < 49)) {
            // above row element c = -1 .. 19, or a copy of an above-right element
            const int c = i < 21 ? i - 1 : 16 + ((i - 37) & 3);
            uint8_t v;
            if (mby == 0) v = 127;
            else if (c < 0) v = mbx > 0 ? Y[-pitch - 1] : 129;
            else if (c < 16 || mbx < mb_w - 1) v = Y[-pitch + c];
            else v = Y[-pitch + 15];
            const int row = i < 21 ? 0 : 4 * (1 + ((i - 37) >> 2));
            w.y[row * kVp8YS + 4 + c] = v;
        } else if (i < 37) {
            const int r = i - 21;
            w.y[(r + 1) * kVp8YS + 3] = mbx > 0 ? Y[(size_t)r * pitch - 1] : 129;
        } else {
            const int j = i - 49, pl = j >= 17 ? 1 : 0, k = j - 17 * pl;     // k 0..8: above c = -1..7; 9..16: left r = 0..7
            uint8_t *t = pl ? w.v : w.u;
            if (k < 9) {
                const int c = k - 1;
                uint8_t v;
                if (mby == 0) v = 127;
                else if (c < 0) v = mbx > 0 ? C[-pitch - 2 + pl] : 129;
                else v = C[-pitch + 2 * c + pl];
                t[4 + c] = v;
            } else {
                const int r = k - 9;
                t[(r + 1) * kVp8CS + 3] = mbx > 0 ? C[(size_t)r * pitch - 2 + pl] : 129;
            }
        }
    }
}

// RFC 6386 12.2: sample (r, c) of an n x n prediction; t points at sample (0, 0) inside a work area of stride st
JR_HD int vp8_pred_mb(int mode, int n, const uint8_t *t, int st, int r, int c, bool has_above, bool has_left) {
    if (mode == VP8_V_PRED) return t[-st + c];
    if (mode == VP8_H_PRED) return t[r * st - 1];
    if (mode == VP8_TM_PRED) return vp8_clamp255(t[r * st - 1] + t[-st + c] - t[-st - 1]);
    const int shift = n == 8 ? 3 : 4;
    int sa = 0, sl = 0;
    for (int i = 0; i < n; i++) { sa += t[-st + i]; sl += t[i * st - 1]; }
    if (has_above && has_left) return (sa + sl + (1 << shift)) >> (shift + 1);
    if (has_above) return (sa + (1 << (shift - 1))) >> shift;
    if (has_left) return (sl + (1 << (shift - 1))) >> shift;
    return 128;
}

// RFC 6386 12.3: sample (r, c) of a 4x4 sub-block prediction.  Edge samples E[0..12]: left column bottom to top, the corner, the 8 above
JR_HD int vp8_pred_b(int mode, const uint8_t *t, int st, int r, int c) {
#define VP8_A(i) ((int)t[-st + (i)])
#define VP8_L(i) ((int)t[(i) * st - 1])
#define VP8_E(i) ((i) < 4 ? VP8_L(3 - (i)) : ((i) == 4 ? (int)t[-st - 1] : VP8_A((i) - 5)))
#define VP8_A3(x, y, z) (((x) + 2 * (y) + (z) + 2) >> 2)
#define VP8_A2(x, y) (((x) + (y) + 1) >> 1)
    switch (mode) {
    case VP8_B_DC: return (VP8_A(0) + VP8_A(1) + VP8_A(2) + VP8_A(3) + VP8_L(0) + VP8_L(1) + VP8_L(2) + VP8_L(3) + 4) >> 3;
    case VP8_B_TM: return vp8_clamp255(VP8_L(r) + VP8_A(c) - (int)t[-st - 1]);
    case VP8_B_VE: return VP8_A3(VP8_E(4 + c), VP8_E(5 + c), VP8_E(6 + c));
    case VP8_B_HE: return r < 3 ? VP8_A3(VP8_E(4 - r), VP8_E(3 - r), VP8_E(2 - r)) : VP8_A3(VP8_L(2), VP8_L(3), VP8_L(3));
    case VP8_B_LD: { const int i = r + c; return VP8_A3(VP8_A(i), VP8_A(i + 1), VP8_A(i + 2 > 7 ? 7 : i + 2)); }
    case VP8_B_RD: { const int i = 4 - r + c; return VP8_A3(VP8_E(i - 1), VP8_E(i), VP8_E(i + 1)); }
    case VP8_B_VR:
        if (r == 0) return VP8_A2(VP8_E(4 + c), VP8_E(5 + c));
        if (r == 1) return VP8_A3(VP8_E(3 + c), VP8_E(4 + c), VP8_E(5 + c));
        if (r == 2) return c == 0 ? VP8_A3(VP8_E(2), VP8_E(3), VP8_E(4)) : VP8_A2(VP8_E(3 + c), VP8_E(4 + c));
        return c == 0 ? VP8_A3(VP8_E(1), VP8_E(2), VP8_E(3)) : VP8_A3(VP8_E(2 + c), VP8_E(3 + c), VP8_E(4 + c));
    case VP8_B_VL:
        if (r == 0) return VP8_A2(VP8_A(c), VP8_A(c + 1));
        if (r == 1) return VP8_A3(VP8_A(c), VP8_A(c + 1), VP8_A(c + 2));
        if (r == 2) return c < 3 ? VP8_A2(VP8_A(c + 1), VP8_A(c + 2)) : VP8_A3(VP8_A(4), VP8_A(5), VP8_A(6));
        return c < 3 ? VP8_A3(VP8_A(c + 1), VP8_A(c + 2), VP8_A(c + 3)) : VP8_A3(VP8_A(5), VP8_A(6), VP8_A(7));
    case VP8_B_HD: {
        if (r == 0 && c >= 2) return VP8_A3(VP8_E(2 + c), VP8_E(3 + c), VP8_E(4 + c));
        const int j = (3 - r) + (c >> 1);
        return (c & 1) ? VP8_A3(VP8_E(j), VP8_E(j + 1), VP8_E(j + 2)) : VP8_A2(VP8_E(j), VP8_E(j + 1));
    }
    default: {      // VP8_B_HU
        const int i = 2 * r + c, j = i >> 1;
        if (j >= 3) return VP8_L(3);
        if (!(i & 1)) return VP8_A2(VP8_L(j), VP8_L(j + 1));
        return VP8_A3(VP8_L(j), VP8_L(j + 1), VP8_L(j + 2 > 3 ? 3 : j + 2));
    }
    }
#undef VP8_A
#undef VP8_L
#undef VP8_E
#undef VP8_A3
#undef VP8_A2
}

// a macroblock that is not B_PRED: lane = row lane >> 2, samples 4 (lane & 3) .. + 3 of the 16x16 prediction, plus residual, into the work area
JR_HD void vp8_luma16_lane(Vp8Work &w, const Vp8Mb &mb, int mbx, int mby, int lane) {
    const int r = lane >> 2, c0 = (lane & 3) * 4;
    const uint8_t *t = w.y + kVp8YS + 4;
    uint8_t px[4];
JR_UNROLL
    for (int k = 0; k < 4; k++) {
        const int c = c0 + k;
        px[k] = vp8_clamp255(vp8_pred_mb(mb.ymode & 3, 16, t, kVp8YS, r, c, mby > 0, mbx > 0) + w.res[(r >> 2) * 4 + (c >> 2)][(r & 3) * 4 + (c & 3)]);
    }
JR_UNROLL
    for (int k = 0; k < 4; k++) w.y[(r + 1) * kVp8YS + 4 + c0 + k] = px[k];
}
// (V_PRED, H_PRED and TM_PRED read only the borders, DC_PRED too: no lane reads what another writes in this phase)

// B_PRED, sub-block k (0..15, in raster order, one phase each) with its mode: lanes 0..15 = its 16 samples.  (A sub-block's prediction reads only
// samples outside the sub-block: no lane reads what another lane writes in this phase.)
JR_HD void vp8_bpred_lane(Vp8Work &w, int mode, int k, int lane) {
    if (lane >= 16) return;
    const int r = lane >> 2, c = lane & 3;
    uint8_t *t = w.y + ((k >> 2) * 4 + 1) * kVp8YS + 4 + (k & 3) * 4;
    if (mode > VP8_B_HU) mode = VP8_B_DC;
    const uint8_t v = vp8_clamp255(vp8_pred_b(mode, t, kVp8YS, r, c) + w.res[k][lane]);
    t[r * kVp8YS + c] = v;
}

// chroma: lane = sample (lane >> 3, lane & 7) of U and of V; returns U | V << 8
JR_HD uint32_t vp8_chroma_lane(const Vp8Work &w, const Vp8Mb &mb, int mbx, int mby, int lane) {
    const int r = lane >> 3, c = lane & 7, b = (r >> 2) * 2 + (c >> 2), e = (r & 3) * 4 + (c & 3);
    const int m = mb.uvmode & 3;
    const uint32_t u = vp8_clamp255(vp8_pred_mb(m, 8, w.u + kVp8CS + 4, kVp8CS, r, c, mby > 0, mbx > 0) + w.res[16 + b][e]);
    const uint32_t v = vp8_clamp255(vp8_pred_mb(m, 8, w.v + kVp8CS + 4, kVp8CS, r, c, mby > 0, mbx > 0) + w.res[20 + b][e]);
    return u | v << 8;
}

// the finished macroblock into the surface: lane = 4 luma samples (row lane >> 2) as one dword, and one U, V pair
JR_HD void vp8_store_lane(const Vp8Work &w, uint8_t *surf, int pitch, int chroma_offset, int mbx, int mby, uint32_t uv, int lane) {
    const int r = lane >> 2, c0 = (lane & 3) * 4;
    const uint8_t *s = &w.y[(r + 1) * kVp8YS + 4 + c0];
    *reinterpret_cast<uint32_t *>(surf + (size_t)(mby * 16 + r) * pitch + mbx * 16 + c0) = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
    *reinterpret_cast<uint16_t *>(surf + chroma_offset + (size_t)(mby * 8 + (lane >> 3)) * pitch + mbx * 16 + 2 * (lane & 7)) = (uint16_t)uv;
}

// ---- the loop filters (RFC 6386 section 15) ------------------------------------------------------------------------------------------------------
JR_HD int vp8_c(int v) { return v < -128 ? -128 : (v > 127 ? 127 : v); }
JR_HD int vp8_abs(int v) { return v < 0 ? -v : v; }

// interior limit, sub-block edge limit, macroblock edge limit and the key-frame hev threshold of a level (15.2, 15.3)
// (inter: the thresholds of frames that are no key frames -- 40 -> 3, 20 -> 2, 15 -> 1)
JR_HD void vp8_filter_limits(int level, int sharpness, int *interior, int *sub_limit, int *mb_limit, int *thresh, int inter = 0) {
    int il = level;
    if (sharpness) { il >>= sharpness > 4 ? 2 : 1; if (il > 9 - sharpness) il = 9 - sharpness; }
    if (il < 1) il = 1;
    *interior = il; *sub_limit = level * 2 + il; *mb_limit = (level + 2) * 2 + il;
    *thresh = inter ? (level >= 40 ? 3 : (level >= 20 ? 2 : (level >= 15 ? 1 : 0))) : (level >= 40 ? 2 : (level >= 15 ? 1 : 0));
}

// p points at q0, samples st apart across the edge
JR_HD int vp8_common_adjust(bool use_outer, uint8_t *p, int st) {
    const int p1 = p[-2 * st] - 128, p0 = p[-st] - 128, q0 = p[0] - 128, q1 = p[st] - 128;
    int a = vp8_c((use_outer ? vp8_c(p1 - q1) : 0) + 3 * (q0 - p0));
    const int b = vp8_c(a + 3) >> 3;
    a = vp8_c(a + 4) >> 3;
    p[0] = (uint8_t)(vp8_c(q0 - a) + 128); p[-st] = (uint8_t)(vp8_c(p0 + b) + 128);
    return a;
}
JR_HD void vp8_filter_simple(uint8_t *p, int st, int limit) {
    if (vp8_abs(p[-st] - p[0]) * 2 + (vp8_abs(p[-2 * st] - p[st]) >> 1) <= limit) vp8_common_adjust(true, p, st);
}
JR_HD bool vp8_filter_yes(const uint8_t *p, int st, int interior, int limit) {
    const int p3 = p[-4 * st], p2 = p[-3 * st], p1 = p[-2 * st], p0 = p[-st], q0 = p[0], q1 = p[st], q2 = p[2 * st], q3 = p[3 * st];
    return vp8_abs(p0 - q0) * 2 + (vp8_abs(p1 - q1) >> 1) <= limit && vp8_abs(p3 - p2) <= interior && vp8_abs(p2 - p1) <= interior &&
           vp8_abs(p1 - p0) <= interior && vp8_abs(q3 - q2) <= interior && vp8_abs(q2 - q1) <= interior && vp8_abs(q1 - q0) <= interior;
}
JR_HD bool vp8_hev(const uint8_t *p, int st, int thresh) { return vp8_abs(p[-2 * st] - p[-st]) > thresh || vp8_abs(p[st] - p[0]) > thresh; }
JR_HD void vp8_filter_subblock(uint8_t *p, int st, int interior, int limit, int thresh) {
    if (!vp8_filter_yes(p, st, interior, limit)) return;
    const bool hv = vp8_hev(p, st, thresh);
    const int p1 = p[-2 * st] - 128, q1 = p[st] - 128;
    const int a = (vp8_common_adjust(hv, p, st) + 1) >> 1;
    if (!hv) { p[st] = (uint8_t)(vp8_c(q1 - a) + 128); p[-2 * st] = (uint8_t)(vp8_c(p1 + a) + 128); }
}
JR_HD void vp8_filter_mbedge(uint8_t *p, int st, int interior, int limit, int thresh) {
    if (!vp8_filter_yes(p, st, interior, limit)) return;
    if (vp8_hev(p, st, thresh)) { vp8_common_adjust(true, p, st); return; }
    const int p2 = p[-3 * st] - 128, p1 = p[-2 * st] - 128, p0 = p[-st] - 128, q0 = p[0] - 128, q1 = p[st] - 128, q2 = p[2 * st] - 128;
    const int w = vp8_c(vp8_c(p1 - q1) + 3 * (q0 - p0));
    int a = vp8_c((27 * w + 63) >> 7);
    p[0] = (uint8_t)(vp8_c(q0 - a) + 128); p[-st] = (uint8_t)(vp8_c(p0 + a) + 128);
    a = vp8_c((18 * w + 63) >> 7);
    p[st] = (uint8_t)(vp8_c(q1 - a) + 128); p[-2 * st] = (uint8_t)(vp8_c(p1 + a) + 128);
    a = vp8_c((9 * w + 63) >> 7);
    p[2 * st] = (uint8_t)(vp8_c(q2 - a) + 128); p[-3 * st] = (uint8_t)(vp8_c(p2 + a) + 128);
}

// The filter work area of one macroblock: the macroblock with the 4 samples to its left and the 4 rows above it (what its edge filters read; they
// write 3 of them).  y: 20 rows of 20 bytes; c: 12 rows of 24 bytes of interleaved U, V (8 bytes = 4 pairs to the left).
constexpr int kVp8FYS = 20, kVp8FCS = 24;
struct Vp8FiltWork { uint8_t y[20 * kVp8FYS]; uint8_t c[12 * kVp8FCS]; };

// load (store == false) or store the work area as dwords: 100 of luma, 72 of chroma.  What lies outside the frame (left of column 0, above row 0) is
// neither read nor written -- and no filter touches those bytes of the work area, since the frame's own edges are not filtered.
JR_HD void vp8_filt_copy_lane(Vp8FiltWork &w, uint8_t *surf, int pitch, int chroma_offset, int mbx, int mby, bool store, int lane) {
    for (int i = lane; i < 172; i += 64) {
        uint32_t *t; uint8_t *g;
        if (i < 100) {
            const int row = i / 5, dw = i - row * 5;
            if ((mby == 0 && row < 4) || (mbx == 0 && dw == 0)) continue;
            t = reinterpret_cast<uint32_t *>(&w.y[row * kVp8FYS + dw * 4]);
            g = surf + ((ptrdiff_t)(mby * 16 - 4 + row)) * pitch + mbx * 16 - 4 + dw * 4;
        } else {
            const int j = i - 100, row = j / 6, dw = j - row * 6;
            if ((mby == 0 && row < 4) || (mbx == 0 && dw < 2)) continue;
            t = reinterpret_cast<uint32_t *>(&w.c[row * kVp8FCS + dw * 4]);
            g = surf + chroma_offset + ((ptrdiff_t)(mby * 8 - 4 + row)) * pitch + mbx * 16 - 8 + dw * 4;
        }
        if (store) *reinterpret_cast<uint32_t *>(g) = *t; else *t = *reinterpret_cast<const uint32_t *>(g);
    }
}

// phase 0: the vertical edges (the macroblock's left edge, then its inner ones, left to right) -- lane = one row: 0..15 luma, 16..31 the rows of U and V;
// phase 1: the horizontal edges (top edge, then the inner ones) -- lane = one column: 0..15 luma, 16..31 the interleaved chroma columns.
// RFC 6386 15: all vertical edges of a macroblock before its horizontal ones; rows (columns) are independent of each other within a phase.
JR_HD void vp8_filter_lane(Vp8FiltWork &w, const Vp8Mb &mb, int filter_type, int sharpness, int mbx, int mby, int phase, int lane, int inter = 0) {
    const int level = mb.level > 63 ? 63 : mb.level;
    if (!level || lane >= 32 || (filter_type && lane >= 16)) return;
    int interior, sub_limit, mb_limit, thresh;
    vp8_filter_limits(level, sharpness, &interior, &sub_limit, &mb_limit, &thresh, inter);
    const bool inner = (mb.flags & VP8_MB_INNER) != 0, edge = phase ? mby > 0 : mbx > 0;
    uint8_t *p; int st, step, n_inner;      // st: across the edge; step: from one edge to the next inner one
    if (lane < 16) {
        p = phase ? &w.y[4 * kVp8FYS + 4 + lane] : &w.y[(4 + lane) * kVp8FYS + 4];
        st = phase ? kVp8FYS : 1; step = 4 * st; n_inner = 3;
    } else {
        const int k = lane - 16;
        p = phase ? &w.c[4 * kVp8FCS + 8 + k] : &w.c[(4 + (k & 7)) * kVp8FCS + 8 + (k >> 3)];
        st = phase ? kVp8FCS : 2; step = 4 * st; n_inner = 1;
    }
    if (edge) { if (filter_type) vp8_filter_simple(p, st, mb_limit); else vp8_filter_mbedge(p, st, interior, mb_limit, thresh); }
    if (inner) for (int e = 1; e <= n_inner; e++) {
        if (filter_type) vp8_filter_simple(p + e * step, st, sub_limit); else vp8_filter_subblock(p + e * step, st, interior, sub_limit, thresh);
    }
}

// ---- inter prediction (RFC 6386 section 18; option vp8_inter) --------------------------------------------------------------------------------------
// A macroblock is predicted in REGIONS, each n x n samples of one plane with one vector: a whole macroblock has 3 (luma 16, U 8, V 8), a SPLITMV
// macroblock 24 (16 luma and 2 x 4 chroma blocks of 4 x 4; blocks with equal vectors give the same samples one by one as together).  Per region the
// (n + 5) x (n + 5) window of the reference -- rows and columns -2 .. n + 2 around the displaced block, coordinates clamped to the decoded area, which
// is the RFC's "as if replicated without end" -- is fetched into the work area, filtered horizontally over all n + 5 rows into tmp (+64 >> 7, clamped
// to 8 bits) and then vertically (the same), the residual added.  Bilinear (versions 1 .. 3) is the same procedure with taps {0, 0, 128 - 16 k, 16 k,
// 0, 0}: its first pass needs row n only, the others meet zero taps.  A fraction of 0 is the tap row {0, 0, 128, 0, 0, 0}: exact.
constexpr int kVp8WinBytes = 24 * 81 + 8, kVp8TmpBytes = 24 * 36;          // (whole macroblock: 441 + 2 x 169 = 779 and 336 + 2 x 104 = 544)
struct Vp8InterWork {
    Vp8Work w;                     // coefficients and residuals as for intra macroblocks; y, u, v take the finished samples
    uint8_t win[kVp8WinBytes];
    uint8_t tmp[kVp8TmpBytes];
    int16_t mv[24][2];             // per region: x, y in eighth samples of its plane
};
struct Vp8Region { int plane, n, bx, by, win, tmp; };      // bx, by: the block inside the macroblock; win, tmp: offsets (strides n + 5 and n)

JR_HD Vp8Region vp8_region(bool split, int r) {
    Vp8Region R;
    if (split) {
        const int q = r < 16 ? r : (r - 16) & 3;
        R.plane = r < 16 ? 0 : (r < 20 ? 1 : 2); R.n = 4;
        R.bx = r < 16 ? (q & 3) * 4 : (q & 1) * 4; R.by = r < 16 ? (q >> 2) * 4 : (q >> 1) * 4;
        R.win = r * 81; R.tmp = r * 36;
    } else {
        R.plane = r; R.n = r ? 8 : 16; R.bx = R.by = 0;
        R.win = r == 0 ? 0 : (r == 1 ? 441 : 610); R.tmp = r == 0 ? 0 : (r == 1 ? 336 : 440);
    }
    return R;
}
// the six taps of fraction f (eighths), for samples -2 .. +3
JR_HD void vp8_taps(int interp, int f, int *t) {
    f &= 7;
    if (interp) { t[0] = t[1] = t[4] = t[5] = 0; t[2] = 128 - 16 * f; t[3] = 16 * f; return; }
    switch (f) {
    case 0: t[0] = 0; t[1] = 0; t[2] = 128; t[3] = 0; t[4] = 0; t[5] = 0; break;
    case 1: t[0] = 0; t[1] = -6; t[2] = 123; t[3] = 12; t[4] = -1; t[5] = 0; break;
    case 2: t[0] = 2; t[1] = -11; t[2] = 108; t[3] = 36; t[4] = -8; t[5] = 1; break;
    case 3: t[0] = 0; t[1] = -9; t[2] = 93; t[3] = 50; t[4] = -6; t[5] = 0; break;
    case 4: t[0] = 3; t[1] = -16; t[2] = 77; t[3] = 77; t[4] = -16; t[5] = 3; break;
    case 5: t[0] = 0; t[1] = -6; t[2] = 50; t[3] = 93; t[4] = -9; t[5] = 0; break;
    case 6: t[0] = 1; t[1] = -8; t[2] = 36; t[3] = 108; t[4] = -11; t[5] = 2; break;
    default: t[0] = 0; t[1] = -1; t[2] = 12; t[3] = 123; t[4] = -6; t[5] = 0; break;
    }
}

// lanes 0..23: the vector of region `lane`.  sv: the macroblock's entry of the picture's split list (SPLITMV), else unused
JR_HD void vp8_inter_mvs_lane(Vp8InterWork &iw, const Vp8InterInfo &ii, const Vp8SplitMv *sv, int lane) {
    const bool split = ii.split != 0 && sv != nullptr;
    if (lane >= (split ? 24 : 3)) return;
    if (split) {
        const int16_t *v = lane < 16 ? sv->y[lane] : sv->c[(lane - 16) & 3];
        iw.mv[lane][0] = v[0]; iw.mv[lane][1] = v[1];
    } else {
        const int lx = ii.mvx, ly = ii.mvy, cx = ii.cmvx, cy = ii.cmvy;      // (values, not a choice between two addresses inside ii: that would put ii into scratch)
        iw.mv[lane][0] = (int16_t)(lane ? cx : lx); iw.mv[lane][1] = (int16_t)(lane ? cy : ly);
    }
}
// the windows.  Reads of ref: luma (x, y) with 0 <= x < 16 mb_w, 0 <= y < 16 mb_h; chroma (x, y) with 0 <= x < 8 mb_w, 0 <= y < 8 mb_h -- whatever the vectors
JR_HD void vp8_inter_fetch_lane(Vp8InterWork &iw, bool split, const uint8_t *ref, int pitch, int chroma_offset, int mb_w, int mb_h, int mbx, int mby, int lane) {
    const int total = split ? 24 * 81 : 779;
    for (int i = lane; i < total; i += 64) {
        const int r = split ? i / 81 : (i < 441 ? 0 : (i < 610 ? 1 : 2));
        const Vp8Region R = vp8_region(split, r);
        const int j = i - R.win, ws = R.n + 5, wy = j / ws, wx = j - wy * ws;
        const int unit = R.plane ? 8 : 16, pw = unit * mb_w, ph = unit * mb_h;
        int x = mbx * unit + R.bx + (iw.mv[r][0] >> 3) - 2 + wx, y = mby * unit + R.by + (iw.mv[r][1] >> 3) - 2 + wy;
        x = x < 0 ? 0 : (x > pw - 1 ? pw - 1 : x); y = y < 0 ? 0 : (y > ph - 1 ? ph - 1 : y);
        iw.win[i] = R.plane ? ref[chroma_offset + (size_t)y * pitch + 2 * x + (R.plane - 1)] : ref[(size_t)y * pitch + x];
    }
}
// first pass: every row of every window, horizontally
JR_HD void vp8_inter_hpass_lane(Vp8InterWork &iw, bool split, int interp, int lane) {
    const int total = split ? 24 * 36 : 544;
    for (int i = lane; i < total; i += 64) {
        const int r = split ? i / 36 : (i < 336 ? 0 : (i < 440 ? 1 : 2));
        const Vp8Region R = vp8_region(split, r);
        const int j = i - R.tmp, row = j / R.n, col = j - row * R.n;
        int t[6];
        vp8_taps(interp, iw.mv[r][0], t);
        const uint8_t *s = &iw.win[R.win + row * (R.n + 5) + col];
        const int sum = s[0] * t[0] + s[1] * t[1] + s[2] * t[2] + s[3] * t[3] + s[4] * t[4] + s[5] * t[5];
        iw.tmp[i] = vp8_clamp255((sum + 64) >> 7);
    }
}
// second pass, vertically, plus the residual (has_res: the macroblock has entries), into w.y / w.u / w.v where vp8_inter_store_lane finds them
JR_HD void vp8_inter_vpass_lane(Vp8InterWork &iw, bool split, int interp, bool has_res, int lane) {
    for (int i = lane; i < 384; i += 64) {
        int r, row, col;
        if (split) { r = i >> 4; row = (i >> 2) & 3; col = i & 3; }
        else if (i < 256) { r = 0; row = i >> 4; col = i & 15; }
        else { r = i < 320 ? 1 : 2; row = (i >> 3) & 7; col = i & 7; }
        const Vp8Region R = vp8_region(split, r);
        int t[6];
        vp8_taps(interp, iw.mv[r][1], t);
        const uint8_t *s = &iw.tmp[R.tmp + row * R.n + col];
        const int n = R.n, sum = s[0] * t[0] + s[n] * t[1] + s[2 * n] * t[2] + s[3 * n] * t[3] + s[4 * n] * t[4] + s[5 * n] * t[5];
        int v = vp8_clamp255((sum + 64) >> 7);
        const int yy = R.by + row, xx = R.bx + col;
        if (has_res) v = vp8_clamp255(v + iw.w.res[R.plane ? 16 + 4 * (R.plane - 1) + (yy >> 2) * 2 + (xx >> 2) : (yy >> 2) * 4 + (xx >> 2)][(yy & 3) * 4 + (xx & 3)]);
        if (R.plane == 0) iw.w.y[(yy + 1) * kVp8YS + 4 + xx] = (uint8_t)v;
        else (R.plane == 1 ? iw.w.u : iw.w.v)[(yy + 1) * kVp8CS + 4 + xx] = (uint8_t)v;
    }
}
JR_HD void vp8_inter_store_lane(const Vp8InterWork &iw, uint8_t *surf, int pitch, int chroma_offset, int mbx, int mby, int lane) {
    const int o = ((lane >> 3) + 1) * kVp8CS + 4 + (lane & 7);
    vp8_store_lane(iw.w, surf, pitch, chroma_offset, mbx, mby, (uint32_t)iw.w.u[o] | (uint32_t)iw.w.v[o] << 8, lane);
}
// the record's Vp8InterInfo, every field the device indexes with clamped: ref 1..3 (0: the picture lacks that reference -- the macroblock is left alone)
// b: the four dwords of the record's bmodes bytes
JR_HD bool vp8_inter_info(const Vp8PicParams &pp, const uint32_t b[4], Vp8InterInfo &ii, const uint8_t *&ref, const Vp8SplitMv *&sv) {
    ii.ref = (uint8_t)(b[0] & 0xff); ii.split = (uint8_t)(b[0] >> 8 & 0xff); ii.pad[0] = ii.pad[1] = 0;
    ii.mvx = (int16_t)(b[1] & 0xffff); ii.mvy = (int16_t)(b[1] >> 16); ii.cmvx = (int16_t)(b[2] & 0xffff); ii.cmvy = (int16_t)(b[2] >> 16); ii.split_idx = b[3];
    if (ii.ref < 1 || ii.ref > 3) return false;
    ref = pp.ref[ii.ref - 1];
    sv = nullptr;
    if (ii.split) { if (!pp.split || ii.split_idx >= (uint32_t)pp.n_split) return false; sv = pp.split + ii.split_idx; }
    return ref != nullptr;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// k_vp8_inter played on the CPU: the macroblocks in raster order (on the device they run side by side: none reads what another writes), per
// macroblock the phases of vp8_kernels.hip with lanes 0..63 in turn
inline void vp8_inter_mb_host(const Vp8PicParams &pp, Vp8InterWork &iw, int mbx, int mby) {
    const Vp8Mb &mb = pp.mbs[(size_t)mby * pp.mb_w + mbx];
    if (!(mb.flags & VP8_MB_INTER)) return;
    Vp8InterInfo ii; const uint8_t *ref; const Vp8SplitMv *sv;
    uint32_t words[4]; memcpy(words, mb.bmodes, 16);
    if (!vp8_inter_info(pp, words, ii, ref, sv)) return;
    const bool split = sv != nullptr, has_res = mb.count != 0;
    if (has_res) {
        for (int l = 0; l < 64; l++) vp8_zero_lane(iw.w, l);
        for (int l = 0; l < 64; l++) vp8_scatter_lane(iw.w, mb, pp.entries, pp.n_entries, pp.dq[mb.segment & 3], l);
        if (mb.ymode != VP8_B_PRED && (mb.nz >> 24 & 1)) for (int l = 0; l < 64; l++) vp8_wht_lane(iw.w, l);
        for (int l = 0; l < 64; l++) vp8_idct_lane(iw.w, mb, l);
    }
    for (int l = 0; l < 64; l++) vp8_inter_mvs_lane(iw, ii, sv, l);
    for (int l = 0; l < 64; l++) vp8_inter_fetch_lane(iw, split, ref, pp.pitch, pp.chroma_offset, pp.mb_w, pp.mb_h, mbx, mby, l);
    for (int l = 0; l < 64; l++) vp8_inter_hpass_lane(iw, split, pp.interp, l);
    for (int l = 0; l < 64; l++) vp8_inter_vpass_lane(iw, split, pp.interp, has_res, l);
    for (int l = 0; l < 64; l++) vp8_inter_store_lane(iw, pp.surf, pp.pitch, pp.chroma_offset, mbx, mby, l);
}
inline void vp8_inter_host(const Vp8PicParams &pp) {
    if (pp.mb_w <= 0 || pp.mb_h <= 0 || !pp.inter) return;
    Vp8InterWork iw;
    for (int y = 0; y < pp.mb_h; y++) for (int x = 0; x < pp.mb_w; x++) vp8_inter_mb_host(pp, iw, x, y);
}

// Host: the two kernels played on the CPU in their own order -- bands of 16 macroblock rows, per band the steps s = 0 .. mb_w + 2 (rows - 1) - 1, per step
// "wave" w = 0..15 with macroblock (s - 2 w, row0 + w), per macroblock the phases of vp8_kernels.hip with lanes 0..63 in turn.  The surface is as
// the device's: pitch a multiple of 4, 16 mb_w x 16 mb_h luma samples, chroma at chroma_offset.
inline void vp8_recon_mb_host(const Vp8PicParams &pp, Vp8Work &w, int mbx, int mby) {
    const Vp8Mb &mb = pp.mbs[(size_t)mby * pp.mb_w + mbx];
    if (mb.flags & VP8_MB_INTER) return;          // (k_vp8_inter has put it on the surface)
    const bool bpred = mb.ymode >= VP8_B_PRED;
    for (int l = 0; l < 64; l++) vp8_zero_lane(w, l);
    for (int l = 0; l < 64; l++) vp8_scatter_lane(w, mb, pp.entries, pp.n_entries, pp.dq[mb.segment & 3], l);
    if (!bpred && (mb.nz >> 24 & 1)) for (int l = 0; l < 64; l++) vp8_wht_lane(w, l);
    for (int l = 0; l < 64; l++) { vp8_idct_lane(w, mb, l); vp8_borders_lane(w, pp.surf, pp.pitch, pp.chroma_offset, mbx, mby, pp.mb_w, l); }
    if (!bpred) for (int l = 0; l < 64; l++) vp8_luma16_lane(w, mb, mbx, mby, l);
    else for (int k = 0; k < 16; k++) for (int l = 0; l < 64; l++) vp8_bpred_lane(w, mb.bmodes[k], k, l);
    uint32_t uv[64];
    for (int l = 0; l < 64; l++) uv[l] = vp8_chroma_lane(w, mb, mbx, mby, l);
    for (int l = 0; l < 64; l++) vp8_store_lane(w, pp.surf, pp.pitch, pp.chroma_offset, mbx, mby, uv[l], l);
}
inline void vp8_filter_mb_host(const Vp8PicParams &pp, Vp8FiltWork &w, int mbx, int mby) {
    const Vp8Mb &mb = pp.mbs[(size_t)mby * pp.mb_w + mbx];
    if (!mb.level) return;
    for (int l = 0; l < 64; l++) vp8_filt_copy_lane(w, pp.surf, pp.pitch, pp.chroma_offset, mbx, mby, false, l);
    for (int ph = 0; ph < 2; ph++) for (int l = 0; l < 64; l++) vp8_filter_lane(w, mb, pp.filter_type, pp.sharpness, mbx, mby, ph, l, pp.inter);
    for (int l = 0; l < 64; l++) vp8_filt_copy_lane(w, pp.surf, pp.pitch, pp.chroma_offset, mbx, mby, true, l);
}
template <class PerMb> inline void vp8_wavefront_host(const Vp8PicParams &pp, PerMb &&per_mb) {
    constexpr int kWaves = 16;
    for (int row0 = 0; row0 < pp.mb_h; row0 += kWaves) {
        const int rows = pp.mb_h - row0 < kWaves ? pp.mb_h - row0 : kWaves;
        for (int s = 0; s < pp.mb_w + 2 * (rows - 1); s++)
            for (int wv = 0; wv < rows; wv++) { const int mbx = s - 2 * wv; if (mbx >= 0 && mbx < pp.mb_w) per_mb(mbx, row0 + wv); }
    }
}
inline void vp8_reconstruct_host(const Vp8PicParams &pp) {
    if (pp.mb_w <= 0 || pp.mb_h <= 0 || (pp.inter && pp.n_intra == 0)) return;
    Vp8Work w;
    vp8_wavefront_host(pp, [&](int x, int y) { vp8_recon_mb_host(pp, w, x, y); });
}
inline void vp8_filter_host(const Vp8PicParams &pp) {
    if (pp.mb_w <= 0 || pp.mb_h <= 0 || !pp.filtered) return;
    Vp8FiltWork w;
    vp8_wavefront_host(pp, [&](int x, int y) { vp8_filter_mb_host(pp, w, x, y); });
}
#endif

}  // namespace jmamd
