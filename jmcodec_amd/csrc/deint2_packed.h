// jmcodec_amd/csrc/deint2_packed.h -- field-rate deinterlacing: D_0(F) and D_1(F) of one surface in one pass (k_deint2, out_kernels.hip).
//
// With option deinterlace_rate = 1 a display frame F leaves as two frames, D with the top rows kept and D with the bottom rows kept (INTEGRATION.md
// "Deinterlaced output").  Every row of F is a kept row of one of them and a missing row of the other, so both come out of ONE walk over the plane:
// a lane owns one 16-byte column chunk and the 8 output rows 8 k .. 8 k + 7, its window is the 10 source rows 8 k - 1 .. 8 k + 8 (window_row: the row
// above the plane is row 1, the row below it row H - 2 -- up() / dn() of the definition for either parity).  Each of the ten rows is loaded once, all of
// them before the first store; row y goes unchanged to the output that keeps its parity and rebuilt to the other one.  Mode 2 computes each vertical
// difference d[y] = P[y] - P[y + 1] once: the negated product of missing row y (comb16, deint_packed.h) is ns[y] = d[y - 1] * d[y], so neighbouring
// rows -- which belong to different outputs -- share a factor.  Decision, byte mask and bit-select are comb16's.
// Against two deint_strip walks this reads 10 rows instead of 2 x 9 (mode 2) per strip and stores the same 16.
// __host__ __device__ like deint_packed.h: tests/test_field_rate_host.py runs this very routine on the CPU (tests/native/deint2_packed_check.cpp).
#pragma once
#include "deint_packed.h"

namespace jmamd {
namespace dei {

JM_HD int strip2_count(int H) { return (H + kDeintStrip - 1) / kDeintStrip; }

// the vertical differences of one row pair, sample q in [-STEP, 16 + STEP) at index q + STEP
template <int STEP> JM_HD void vdiff16(const Chunk &a, uint32_t ea, const Chunk &b, uint32_t eb, int *d) {
    JM_DEI_UNROLL
    for (int q = -STEP; q < 16 + STEP; q++) d[q + STEP] = sample_at(a, ea, q) - sample_at(b, eb, q);
}
// mode 2 from the two differences around the missing row: ns = da * db, then comb16's decision (thr = 4 T^2) between the average of up / dn and cur
template <int STEP> JM_HD Chunk comb16_d(const int *da, const int *db, const Chunk &up, const Chunk &cur, const Chunk &dn, int thr) {
    int ns[16 + 2 * STEP];
    JM_DEI_UNROLL
    for (int q = 0; q < 16 + 2 * STEP; q++) ns[q] = da[q] * db[q];          // -s: |ns| <= 65025
    Chunk o;
    JM_DEI_UNROLL
    for (int k = 0; k < 4; k++) {
        uint32_t t[4];
        for (int j = 0; j < 4; j++) { const int x = 4 * k + j + STEP; t[j] = (uint32_t)(thr + ns[x - STEP] + ns[x + STEP] + 2 * ns[x]); }    // < 0: combed
        const uint32_t m01 = pk::perm(t[1], t[0], 0x0c0c0703u), m23 = pk::perm(t[3], t[2], 0x0c0c0703u);
        const uint32_t mask = pk::perm(m23, m01, 0x05040100u);
        o.w[k] = bfi(mask, pk::lerp(up.w[k], dn.w[k], pk::kOnes), cur.w[k]);
    }
    return o;
}

// a whole chunk of aligned rows: o0 / o1 is the output that keeps the even / the odd rows
template <int STEP, bool COMB> JM_HD void deint2_strip_fast(const gbyte *plane, int pitch, int W, int H, int x, int y0, int thr, const PlaneOut &o0,
                                                            const PlaneOut &o1) {
    Chunk win[kDeintStrip + 2]; uint32_t edge[kDeintStrip + 2];
    JM_DEI_UNROLL
    for (int j = 0; j < kDeintStrip + 2; j++) {
        const gbyte *row = plane + (size_t)window_row(y0 - 1 + j, H) * pitch;
        win[j] = load16<STEP, true>(row, x, 16);
        edge[j] = COMB ? edge16<STEP, true>(row, x, W, win[j]) : 0u;
    }
    int d[2][16 + 2 * STEP];                               // d[j & 1]: slot j minus slot j + 1
    if (COMB) vdiff16<STEP>(win[0], edge[0], win[1], edge[1], d[0]);
    JM_DEI_UNROLL
    for (int j = 1; j <= kDeintStrip; j++) {
        const int y = y0 + j - 1;                          // (y0 is even: row y has the parity of j - 1)
        if (COMB) vdiff16<STEP>(win[j], edge[j], win[j + 1], edge[j + 1], d[j & 1]);
        if (y >= H) continue;
        const PlaneOut &keep = (j & 1) ? o0 : o1, &other = (j & 1) ? o1 : o0;
        store16<true>(keep, y, x, 16, win[j]);
        if (COMB) store16<true>(other, y, x, 16, comb16_d<STEP>(d[(j - 1) & 1], d[j & 1], win[j - 1], win[j], win[j + 1], thr));
        else store16<true>(other, y, x, 16, bob16(win[j - 1], win[j + 1]));
    }
}
// any chunk: byte loads and stores, row by row; row y is kept in `keep` and rebuilt in `other`
template <int STEP> JM_HD void deint2_row_slow(const gbyte *plane, int pitch, int W, int H, int x, int n, int y, int mode, int thr, const PlaneOut &keep,
                                               const PlaneOut &other) {
    const gbyte *row = plane + (size_t)y * pitch, *ru = plane + (size_t)window_row(y - 1, H) * pitch, *rd = plane + (size_t)window_row(y + 1, H) * pitch;
    const Chunk up = load16<STEP, false>(ru, x, n), cur = load16<STEP, false>(row, x, n), dn = load16<STEP, false>(rd, x, n);
    store16<false>(keep, y, x, n, cur);
    if (mode != 2) { store16<false>(other, y, x, n, bob16(up, dn)); return; }
    store16<false>(other, y, x, n, comb16<STEP>(up, cur, dn, edge16<STEP, false>(ru, x, W, up), edge16<STEP, false>(row, x, W, cur),
        edge16<STEP, false>(rd, x, W, dn), thr));
}
template <int STEP> JM_HD void deint2_strip_slow(const gbyte *plane, int pitch, int W, int H, int x, int y0, int mode, int thr, const PlaneOut &o0,
                                                 const PlaneOut &o1) {
    const int n = W - x < 16 ? W - x : 16;
    JM_DEI_ROLLED
    for (int y = y0; y < y0 + kDeintStrip && y < H; y += 2) {
        deint2_row_slow<STEP>(plane, pitch, W, H, x, n, y, mode, thr, o0, o1);
        if (y + 1 < H) deint2_row_slow<STEP>(plane, pitch, W, H, x, n, y + 1, mode, thr, o1, o0);
    }
}
JM_HD bool out_aligned(const PlaneOut &o) {
    return (o.split ? ((uintptr_t)o.d0 | (uintptr_t)o.d1 | (uintptr_t)o.pitch) & 7 : ((uintptr_t)o.d0 | (uintptr_t)o.pitch) & 15) == 0;
}
// strip k (rows 8 k .. 8 k + 7) of the chunk at x of a plane of H rows (H >= 2) and W bytes per row: mode 1 / 2, both outputs
template <int STEP> JM_HD void deint2_strip(const gbyte *plane, int pitch, int W, int H, int x, int k, int mode, int thr, const PlaneOut &o0,
                                            const PlaneOut &o1) {
    const int y0 = k * kDeintStrip;
    const bool aligned = (((uintptr_t)plane | (uintptr_t)pitch) & 15) == 0 && out_aligned(o0) && out_aligned(o1);
    if (W - x >= 16 && aligned) {
        if (mode == 2) deint2_strip_fast<STEP, true>(plane, pitch, W, H, x, y0, thr, o0, o1);
        else deint2_strip_fast<STEP, false>(plane, pitch, W, H, x, y0, thr, o0, o1);
    } else deint2_strip_slow<STEP>(plane, pitch, W, H, x, y0, mode, thr, o0, o1);
}

// A whole frame as k_deint2 sees it: work item i of frame2_items(w, h), ordered like deint_item's.  dst_top / dst_bot: the frames that keep the top /
// the bottom rows, both in the layout deint_item writes (NV12 at dst_pitch / dst_chroma_offset, or a tight I420 frame).
JM_HD int frame2_items(int w, int h) { return ((w + 15) >> 4) * (strip2_count(h) + strip2_count(h >> 1)); }
JM_HD PlaneOut frame_plane(gbyte *dst, bool chroma, int w, int h, int dst_pitch, int dst_chroma_offset, int out_fmt) {
    if (!chroma) return PlaneOut{dst, nullptr, out_fmt == 0 ? dst_pitch : w, false};
    if (out_fmt == 0) return PlaneOut{dst + dst_chroma_offset, nullptr, dst_pitch, false};
    gbyte *u = dst + (size_t)w * h;
    return PlaneOut{u, u + (size_t)(w >> 1) * (h >> 1), w >> 1, true};
}
JM_HD void deint2_item(const gbyte *src, gbyte *dst_top, gbyte *dst_bot, int pitch, int chroma_offset, int w, int h, int dst_pitch, int dst_chroma_offset,
                       int out_fmt, int mode, int thr, int i) {
    const int cpr = (w + 15) >> 4, nl = cpr * strip2_count(h);
    const bool chroma = i >= nl;
    const int j = chroma ? i - nl : i, x = (j % cpr) * 16, k = j / cpr;
    const PlaneOut o0 = frame_plane(dst_top, chroma, w, h, dst_pitch, dst_chroma_offset, out_fmt);
    const PlaneOut o1 = frame_plane(dst_bot, chroma, w, h, dst_pitch, dst_chroma_offset, out_fmt);
    if (!chroma) deint2_strip<1>(src, pitch, w, h, x, k, mode, thr, o0, o1);
    else deint2_strip<2>(src + chroma_offset, pitch, w, h >> 1, x, k, mode, thr, o0, o1);
}

}  // namespace dei
}  // namespace jmamd
