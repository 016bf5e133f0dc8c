// jmcodec_amd/csrc/deint3_packed.h -- the motion-adaptive deinterlacer D3 of INTEGRATION.md "Deinterlaced output" on 16-byte column chunks (k_deint3,
// out_kernels.hip).
//
// D3 keeps the rows of one parity of the plane P and rebuilds the others: a missing sample is the rounded average i of the kept rows above and below where
// something MOVED against the same plane Q of the previous display frame, and the frame's own (woven) sample elsewhere.  m[r][x] = |P[r][x] - Q[r][x]| > T;
// a missing sample at (y, x) has moved when any m in the 3 x 3 neighbourhood up(y) / y / dn(y), cx(x - 1) / x / cx(x + 1) is set.
// A lane owns one 16-byte chunk of a plane and the 8 rows 8 k .. 8 k + 7 (deint2_packed.h's strips); its window is the 10 rows 8 k - 1 .. 8 k + 8 of P in
// registers.  A row of Q is loaded, reduced to the row's mask and dropped:
//   * four samples at a time, in two 16-bit lanes each for the even and the odd bytes: with K = 0x200 - (T + 1) per lane, bit 9 of K + (a - b) is set iff
//     a > b + T and bit 9 of K - (a - b) iff b > a + T (every lane stays inside 1 .. 765, so plain 32-bit adds never carry between lanes): moved4;
//   * one bit per byte, so the masks of the chunk's four words and of its edge word (the STEP samples on either side, edge16 of deint_packed.h applied
//     to P and Q alike) share ONE register per row: bit k of byte b = sample 4 k + b, bit 4 = the edge word (rowmask).  At the plane's edges cx()
//     repeats the edge sample, whose mask is already part of the OR;
//   * a missing row ORs the three rows' registers (v_or3_b32), unpacks five words, ORs each with its neighbours STEP bytes to the left and right
//     (v_alignbit_b32), widens bit 0 of every byte to the byte and bit-selects between one v_lerp_u8 and the woven word, as comb16 does (weave3).
// A job with two destinations (field rate) writes D3 with either parity kept from the same window: every row is a kept row of one output and a missing
// row of the other, and a row's mask serves both.  A job with one destination loads nine of the ten rows.
// __host__ __device__ like deint_packed.h: tests/test_deint3_host.py runs this very routine on the CPU (tests/native/deint3_packed_check.cpp) against a
// numpy restatement of the definition, and tools/deint3_asan.cpp walks it under the sanitizers.
#pragma once
#include "deint2_packed.h"

namespace jmamd {
namespace dei {

constexpr uint32_t kByteBit = 0x01010101u;

JM_HD uint32_t move_k(int T) { return 0x02000200u - (uint32_t)(T + 1) * 0x00010001u; }      // T in 1 .. 255
// bit 0 of every byte: |a - b| > T for that byte, K = move_k(T)
JM_HD uint32_t moved4(uint32_t a, uint32_t b, uint32_t K) {
    const uint32_t dl = (a & 0x00ff00ffu) - (b & 0x00ff00ffu), dh = ((a >> 8) & 0x00ff00ffu) - ((b >> 8) & 0x00ff00ffu);
    const uint32_t gl = (K + dl) | (K - dl), gh = (K + dh) | (K - dh);
    return ((gl >> 9) & 0x00010001u) | ((gh >> 1) & 0x01000100u);
}
// the mask of one row: the chunks p / q of P and Q with their edge words
JM_HD uint32_t rowmask(const Chunk &p, const Chunk &q, uint32_t ep, uint32_t eq, uint32_t K) {
    return moved4(p.w[0], q.w[0], K) | moved4(p.w[1], q.w[1], K) << 1 | moved4(p.w[2], q.w[2], K) << 2 | moved4(p.w[3], q.w[3], K) << 3 | moved4(ep, eq, K) << 4;
}
// a missing row: v = the OR of the masks of the rows above, at and below it
template <int STEP> JM_HD Chunk weave3(uint32_t v, const Chunk &up, const Chunk &cur, const Chunk &dn) {
    const uint32_t e = (v >> 4) & kByteBit;
    // m[1 .. 4]: the chunk's words; m[0] / m[5]: the samples left of it in the top bytes / right of it in the bottom bytes (edge16's layout)
    const uint32_t m[6] = {e << 16, v & kByteBit, (v >> 1) & kByteBit, (v >> 2) & kByteBit, (v >> 3) & kByteBit, e >> 16};
    Chunk o;
    JM_DEI_UNROLL
    for (int k = 0; k < 4; k++) {
        const uint32_t l = m[k + 1] << (8 * STEP) | m[k] >> (32 - 8 * STEP), r = m[k + 1] >> (8 * STEP) | m[k + 2] << (32 - 8 * STEP);
        const uint32_t h = m[k + 1] | l | r;
        o.w[k] = bfi((h << 8) - h, pk::lerp(up.w[k], dn.w[k], pk::kOnes), cur.w[k]);              // (bit 0 of a byte -> 0xFF)
    }
    return o;
}

// a whole chunk of aligned rows (P, Q and the destinations): 16-byte loads, all of them before the first store.  o0 / o1: the outputs that keep the
// even / the odd rows; BOTH: two outputs, else only the one that keeps parity p is written (and the row no missing row of it looks at is not loaded)
template <int STEP, bool BOTH> JM_HD void deint3_strip_fast(const gbyte *plane, int pitch, const gbyte *prev, int prev_pitch, int W, int H, int x, int y0,
                                                            int p, uint32_t K, const PlaneOut &o0, const PlaneOut &o1) {
    Chunk win[kDeintStrip + 2]; uint32_t mask[kDeintStrip + 2];
    JM_DEI_UNROLL
    for (int j = 0; j < kDeintStrip + 2; j++) {
        if (!BOTH && j == (p ? kDeintStrip + 1 : 0)) { win[j] = Chunk{{0, 0, 0, 0}}; mask[j] = 0; continue; }      // (uniform per workgroup)
        const int y = window_row(y0 - 1 + j, H);
        const gbyte *row = plane + (size_t)y * pitch, *qrow = prev + (size_t)y * prev_pitch;
        win[j] = load16<STEP, true>(row, x, 16);
        const Chunk q = load16<STEP, true>(qrow, x, 16);
        mask[j] = rowmask(win[j], q, edge16<STEP, true>(row, x, W, win[j]), edge16<STEP, true>(qrow, x, W, q), K);
    }
    JM_DEI_UNROLL
    for (int j = 1; j <= kDeintStrip; j++) {
        const int y = y0 + j - 1;                          // (y0 is even: row y has the parity of j - 1)
        if (y >= H) continue;
        const PlaneOut &keep = (j & 1) ? o0 : o1, &other = (j & 1) ? o1 : o0;
        const bool kept = ((j - 1) & 1) == p;
        if (BOTH || kept) store16<true>(keep, y, x, 16, win[j]);
        if (BOTH || !kept) store16<true>(other, y, x, 16, weave3<STEP>(mask[j - 1] | mask[j] | mask[j + 1], win[j - 1], win[j], win[j + 1]));
    }
}
// any chunk: byte loads and stores, row by row; the missing row y of `out`
template <int STEP> JM_HD void deint3_row_slow(const gbyte *plane, int pitch, const gbyte *prev, int prev_pitch, int W, int H, int x, int n, int y, uint32_t K,
                                               const PlaneOut &out) {
    const int yu = window_row(y - 1, H), yd = window_row(y + 1, H);
    const gbyte *row = plane + (size_t)y * pitch, *ru = plane + (size_t)yu * pitch, *rd = plane + (size_t)yd * pitch;
    const Chunk up = load16<STEP, false>(ru, x, n), cur = load16<STEP, false>(row, x, n), dn = load16<STEP, false>(rd, x, n);
    uint32_t v = 0;
    {   const gbyte *q = prev + (size_t)yu * prev_pitch; const Chunk c = load16<STEP, false>(q, x, n);
        v |= rowmask(up, c, edge16<STEP, false>(ru, x, W, up), edge16<STEP, false>(q, x, W, c), K); }
    {   const gbyte *q = prev + (size_t)y * prev_pitch; const Chunk c = load16<STEP, false>(q, x, n);
        v |= rowmask(cur, c, edge16<STEP, false>(row, x, W, cur), edge16<STEP, false>(q, x, W, c), K); }
    {   const gbyte *q = prev + (size_t)yd * prev_pitch; const Chunk c = load16<STEP, false>(q, x, n);
        v |= rowmask(dn, c, edge16<STEP, false>(rd, x, W, dn), edge16<STEP, false>(q, x, W, c), K); }
    store16<false>(out, y, x, n, weave3<STEP>(v, up, cur, dn));
}
template <int STEP> JM_HD void deint3_strip_slow(const gbyte *plane, int pitch, const gbyte *prev, int prev_pitch, int W, int H, int x, int y0, int p, bool both,
                                                 uint32_t K, const PlaneOut &o0, const PlaneOut &o1) {
    const int n = W - x < 16 ? W - x : 16;
    JM_DEI_ROLLED
    for (int y = y0; y < y0 + kDeintStrip && y < H; y++) {
        const PlaneOut &keep = (y & 1) ? o1 : o0, &other = (y & 1) ? o0 : o1;
        const bool kept = (y & 1) == p;
        if (both || kept) store16<false>(keep, y, x, n, load16<STEP, false>(plane + (size_t)y * pitch, x, n));
        if (both || !kept) deint3_row_slow<STEP>(plane, pitch, prev, prev_pitch, W, H, x, n, y, K, other);
    }
}
// strip k (rows 8 k .. 8 k + 7) of the chunk at x of a plane of H rows (H >= 2) and W bytes per row, against the same plane `prev` of the previous
// frame.  both: o0 / o1 keep the even / the odd rows; else only the output that keeps parity p is written (the other PlaneOut is not touched)
template <int STEP> JM_HD void deint3_strip(const gbyte *plane, int pitch, const gbyte *prev, int prev_pitch, int W, int H, int x, int k, int p, bool both, int T,
                                            const PlaneOut &o0, const PlaneOut &o1) {
    const int y0 = k * kDeintStrip;
    const uint32_t K = move_k(T);
    const bool aligned = (((uintptr_t)plane | (uintptr_t)pitch | (uintptr_t)prev | (uintptr_t)prev_pitch) & 15) == 0 &&
        (both || !p ? out_aligned(o0) : true) && (both || p ? out_aligned(o1) : true);
    if (W - x >= 16 && aligned) {
        if (both) deint3_strip_fast<STEP, true>(plane, pitch, prev, prev_pitch, W, H, x, y0, p, K, o0, o1);
        else deint3_strip_fast<STEP, false>(plane, pitch, prev, prev_pitch, W, H, x, y0, p, K, o0, o1);
    } else deint3_strip_slow<STEP>(plane, pitch, prev, prev_pitch, W, H, x, y0, p, both, K, o0, o1);
}

// A whole frame as k_deint3 sees it: work item i of frame2_items(w, h), ordered like deint2_item's.  dst keeps `parity`; dst2 (may be null: one
// output) keeps the other one.  Both in the layout deint_item writes.
JM_HD void deint3_item(const gbyte *src, const gbyte *prev, gbyte *dst, gbyte *dst2, int pitch, int chroma_offset, int prev_pitch, int prev_chroma_offset,
                       int w, int h, int dst_pitch, int dst_chroma_offset, int out_fmt, int parity, int T, int i) {
    const int cpr = (w + 15) >> 4, nl = cpr * strip2_count(h);
    const bool chroma = i >= nl, both = dst2 != nullptr;
    const int j = chroma ? i - nl : i, x = (j % cpr) * 16, k = j / cpr;
    gbyte *top = parity ? dst2 : dst, *bot = parity ? dst : dst2;              // (one output: the other one is null and never written)
    const PlaneOut o0 = frame_plane(top ? top : bot, chroma, w, h, dst_pitch, dst_chroma_offset, out_fmt);
    const PlaneOut o1 = frame_plane(bot ? bot : top, chroma, w, h, dst_pitch, dst_chroma_offset, out_fmt);
    if (!chroma) deint3_strip<1>(src, pitch, prev, prev_pitch, w, h, x, k, parity, both, T, o0, o1);
    else deint3_strip<2>(src + chroma_offset, pitch, prev + prev_chroma_offset, prev_pitch, w, h >> 1, x, k, parity, both, T, o0, o1);
}

}  // namespace dei
}  // namespace jmamd
