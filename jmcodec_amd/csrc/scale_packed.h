// jmcodec_amd/csrc/scale_packed.h -- the resampler R_G of INTEGRATION.md "Scaled and cropped output", once (k_scale_pack, k_rgb_pack, out_kernels.hip).
//
// Output = R_G(F), F = the frame k_packout would produce (lone-field row mapping included): separable fixed-point filter, horizontal pass
// h = (sum wx * p + 64) >> 7 (int16), vertical pass out = min(255, (sum wy * h + 2^20) >> 21), taps from the handle's tables (ScaleAxis, jobs.h).
// A workgroup of 256 lanes makes one output tile of one plane: 64 luma columns x 16 rows, or 32 chroma columns (both channels) x 16 chroma rows.  The
// horizontal pass writes the tile's filtered source rows (every row its vertical taps reach) into an int16 buffer of 64 columns per row (LDS), the
// vertical pass reads it.  k_scale_pack runs the two passes per plane and stores 4 output bytes per lane; k_rgb_pack runs the same passes for the luma
// and the chroma of one tile and converts (rgb_packed.h), so its G is k_scale_pack's by construction.
// Everything is __host__ __device__ and one lane's work, the lane index a parameter: a host loop over 256 lanes plays a workgroup, the end of the loop
// a barrier.  tests/test_scaled_output_host.py walks whole frames through these very routines on the CPU (tests/native/scale_packed_check.cpp) and
// compares with the numpy restatement of R_G; tools/out_packed_asan.cpp runs them under AddressSanitizer / UBSan on buffers of the exact size.
// Placed output (INTEGRATION.md "Placed output"; ScaleJob::rx .. fill): the picture is resampled into a rectangle of the target and the rest of the
// target is a fill colour.  Tiles stay on the target grid; plane_tile intersects the tile with the rectangle, the passes run over that share only
// (an empty share reads neither table nor source), and the store merges the fill bytes of a lane with its picture bytes.  rw == 0 is no placement:
// the share is the whole tile and every routine does what it did.  tests/test_placed_output_host.py, tools/place_packed_asan.cpp.
#pragma once
#include "jobs.h"
#include "mc_packed.h"      // JM_HD
#include <string.h>
#include <vector>

namespace jmamd {
namespace scl {

#if defined(__HIP_DEVICE_COMPILE__)
#define JM_SCL_UNROLL _Pragma("unroll")
#else
#define JM_SCL_UNROLL
#endif

constexpr int kScaleTileW = 64, kScaleTileH = 16;      // k_scale_pack: output tile of one plane (chroma: 32 columns x (U, V))
// source rows one tile can reach: 15 output rows of at most 8 source rows each + 1 (floor), + kScaleMaxTaps - 1, + 1; with slack
constexpr int kScaleMaxRows = 136;
constexpr int kRgbTileW = 64, kRgbTileH = 16;          // k_rgb_pack: output tile in pixels; its chroma is 32 x 8 x (U, V)
static_assert(kRgbTileW == kScaleTileW, "both kernels' row buffers are kScaleTileW columns wide");

JM_HD int imin(int a, int b) { return a < b ? a : b; }
JM_HD int imax(int a, int b) { return a > b ? a : b; }
JM_HD int clamp_to(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
// display row -> surface row (a frame of which only one field was decoded: every row shows the line of that parity of its line pair)
JM_HD int surface_row(int row, int lone) { return lone ? ((row & ~1) | (lone - 1)) : row; }
// one sample of 4 / 2 bytes to an address aligned to its size
JM_HD void store_u32(uint8_t *d, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint32_t *)d = v;
#else
    memcpy(d, &v, 4);
#endif
}
JM_HD void store_u16(uint8_t *d, uint16_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint16_t *)d = v;
#else
    memcpy(d, &v, 2);
#endif
}

JM_HD int tiles(int tw, int th) {                      // k_scale_pack's grid: luma tiles, then chroma tiles
    return ((tw + kScaleTileW - 1) / kScaleTileW) * ((th + kScaleTileH - 1) / kScaleTileH) +
           ((tw / 2 + kScaleTileW / 2 - 1) / (kScaleTileW / 2)) * ((th / 2 + kScaleTileH - 1) / kScaleTileH);
}
JM_HD int rgb_tiles(int tw, int th) { return ((tw + kRgbTileW - 1) / kRgbTileW) * ((th + kRgbTileH - 1) / kRgbTileH); }

// One output tile of one plane: output columns j0 .. j0 + jn - 1 and rows i0 .. i0 + in - 1 (chroma: of the half-resolution grid, a column is a (U, V)
// pair), and the source rows r0 .. r0 + nrows - 1 of the crop rectangle that the tile's vertical taps reach
struct PlaneTile {
    const uint8_t *plane; int pitch, lone; bool chroma;
    ScaleAxis ax, ay;
    int ox, oy;                                        // origin of the crop rectangle in the plane's samples
    int j0, i0, jn, in, r0, nrows;
    // Placed output: the tile stays on the target grid; the picture's rectangle starts at (dx, dy) of the plane and the tile's share of it is columns
    // ja .. jb - 1, rows ia .. ib - 1 (target coordinates; unplaced: the whole tile, dx = dy = 0).  The tap tables are indexed by column - dx, row - dy
    // and only ever inside that share; an empty share (ja == jb, nrows == 0) reads neither table nor source.
    bool placed; int dx, dy, ja, jb, ia, ib;
};
// false: the tile's rows do not fit the buffer (cannot happen within the validated ratios: S <= 8 D)
JM_HD bool plane_tile(const ScaleJob &jb, bool chroma, int j0, int i0, int jn, int in, PlaneTile &t) {
    t.plane = jb.src + (chroma ? jb.chroma_offset : 0); t.pitch = jb.pitch; t.lone = jb.lone_field; t.chroma = chroma;
    t.ax = jb.ax[chroma ? 2 : 0]; t.ay = jb.ax[chroma ? 3 : 1];
    t.ox = chroma ? jb.crop_x >> 1 : jb.crop_x; t.oy = chroma ? jb.crop_y >> 1 : jb.crop_y;
    t.j0 = j0; t.i0 = i0; t.jn = jn; t.in = in;
    t.placed = jb.rw != 0; t.dx = t.dy = 0; t.ja = j0; t.jb = j0 + jn; t.ia = i0; t.ib = i0 + in;
    if (t.placed) {                                    // (uniform per workgroup)
        const int sh = chroma ? 1 : 0;
        t.dx = jb.rx >> sh; t.dy = jb.ry >> sh;
        t.ja = imax(j0, t.dx); t.jb = imin(j0 + jn, t.dx + (jb.rw >> sh));
        t.ia = imax(i0, t.dy); t.ib = imin(i0 + in, t.dy + (jb.rh >> sh));
        if (t.ja >= t.jb || t.ia >= t.ib) { t.ja = t.jb = j0; t.ia = t.ib = i0; t.r0 = 0; t.nrows = 0; return true; }     // fill only
    }
    // (clamping is monotonic: every tap of the tile lies in [r0, r1])
    const int Sy = t.ay.src_len;
    t.r0 = clamp_to(t.ay.first[t.ia - t.dy], Sy);
    t.nrows = clamp_to(t.ay.first[t.ib - 1 - t.dy] + t.ay.taps - 1, Sy) - t.r0 + 1;
    return t.nrows <= kScaleMaxRows;
}
// tile t of k_scale_pack's grid; false: no such tile of this job (the grid is sized for the largest job)
JM_HD bool scale_tile(const ScaleJob &jb, int t, PlaneTile &pt) {
    const int tw = jb.tw, th = jb.th, cw = tw >> 1, ch = th >> 1;
    const int txl = (tw + kScaleTileW - 1) / kScaleTileW, nl = txl * ((th + kScaleTileH - 1) / kScaleTileH);
    const int txc = (cw + kScaleTileW / 2 - 1) / (kScaleTileW / 2), nc = txc * ((ch + kScaleTileH - 1) / kScaleTileH);
    if (t >= nl + nc) return false;
    const bool chroma = t >= nl;
    if (chroma) t -= nl;
    const int ntx = chroma ? txc : txl, cols = chroma ? kScaleTileW / 2 : kScaleTileW;
    const int ow = chroma ? cw : tw, oh = chroma ? ch : th;
    const int j0 = (t % ntx) * cols, i0 = (t / ntx) * kScaleTileH;
    return plane_tile(jb, chroma, j0, i0, imin(cols, ow - j0), imin(kScaleTileH, oh - i0), pt);
}

// Horizontal pass of lane tid: buffer column c = tid & 63 is output column c (luma) or output chroma column c / 2, channel c & 1; rows tid / 64, + 4, ...
// PLACED = t.placed, a constant where the caller has branched on it (uniform per workgroup): an unplaced job then runs no placement arithmetic at all
template <bool PLACED> JM_HD void hpass_lane_t(const PlaneTile &t, int tid, int16_t *hbuf) {
    const int c = tid & (kScaleTileW - 1);
    const int jj = t.chroma ? c >> 1 : c;
    if (PLACED ? (t.j0 + jj < t.ja || t.j0 + jj >= t.jb) : jj >= t.jn) return;
    const int j = t.j0 + jj - (PLACED ? t.dx : 0), f = t.ax.first[j], T = t.ax.taps, Sx = t.ax.src_len;
    int xs[kScaleMaxTaps], wv[kScaleMaxTaps];
    JM_SCL_UNROLL
    for (int k = 0; k < kScaleMaxTaps; k++) {
        const int x = t.ox + clamp_to(f + k, Sx);
        xs[k] = t.chroma ? 2 * x + (c & 1) : x;
        wv[k] = k < T ? t.ax.w[j * T + k] : 0;
    }
    for (int r = tid >> 6; r < t.nrows; r += 4) {
        const uint8_t *p = t.plane + (size_t)surface_row(t.oy + t.r0 + r, t.lone) * t.pitch;      // row of the display frame F -> row of the surface
        int acc = 64;
        JM_SCL_UNROLL
        for (int k = 0; k < kScaleMaxTaps; k++) if (k < T) acc += wv[k] * p[xs[k]];
        hbuf[r * kScaleTileW + c] = (int16_t)(acc >> 7);
    }
}
JM_HD void hpass_lane(const PlaneTile &t, int tid, int16_t *hbuf) { if (t.placed) hpass_lane_t<true>(t, tid, hbuf); else hpass_lane_t<false>(t, tid, hbuf); }

// Vertical pass: output row i of the plane (a row of the tile's share of the picture: ia <= i < ib) at the N buffer columns col[].  PLACED = false
// only for a tile that is known to be unplaced (dy == 0)
template <int N, bool PLACED = true> JM_HD void vpass(const PlaneTile &t, int i, const int16_t *hbuf, const int *col, int *out) {
    if (PLACED) i -= t.dy;
    const int fy = t.ay.first[i], Ty = t.ay.taps, Sy = t.ay.src_len;
    int acc[N];
    JM_SCL_UNROLL
    for (int e = 0; e < N; e++) acc[e] = 1 << 20;
    JM_SCL_UNROLL
    for (int k = 0; k < kScaleMaxTaps; k++) {
        if (k >= Ty) break;
        const int w = t.ay.w[i * Ty + k];
        const int16_t *hr = hbuf + (clamp_to(fy + k, Sy) - t.r0) * kScaleTileW;
        JM_SCL_UNROLL
        for (int e = 0; e < N; e++) acc[e] += w * hr[col[e]];
    }
    JM_SCL_UNROLL
    for (int e = 0; e < N; e++) out[e] = imin(255, acc[e] >> 21);
}

// k_scale_pack's vertical pass and store of lane tid: 16 lanes per output row, 4 output bytes each (luma / NV12 chroma: bytes 4q..4q+3 of the tile's
// row = buffer columns 4q..4q+3; I420 chroma: lanes q < 8 write U columns 4q.., lanes q >= 8 V columns 4(q-8).., i.e. buffer columns 2 * column + channel).
// A placed job: the bytes outside the tile's share of the picture are the fill of their plane; the lane still stores its 4 bytes once.
template <bool PLACED> JM_HD void vpass_store_lane_t(const ScaleJob &jb, const PlaneTile &t, int tid, const int16_t *hbuf) {
    const int r = tid >> 4, q = tid & 15;
    if (r >= t.in) return;
    const int i = t.i0 + r, tw = jb.tw, th = jb.th, cw = tw >> 1, ch = th >> 1;
    const bool chroma = t.chroma, planar = chroma && jb.out_fmt == 1;
    int col[4], n_valid = 0;
    uint32_t inside = 15, fill = 0;                                   // bit e: byte e is a sample of the picture; the fill bytes of the lane
    JM_SCL_UNROLL
    for (int e = 0; e < 4; e++) {
        const int b = planar ? 4 * (q & 7) + e : 4 * q + e;          // output byte of the tile's row (planar: in its U or V row)
        col[e] = planar ? 2 * b + (q >> 3) : b;
        if ((planar ? b : (chroma ? b >> 1 : b)) < t.jn) n_valid = e + 1;
    }
    if (PLACED) {
        int any = -1;
        JM_SCL_UNROLL
        for (int e = 0; e < 4; e++) {
            const int b = planar ? 4 * (q & 7) + e : 4 * q + e, j = t.j0 + (planar ? b : (chroma ? b >> 1 : b));
            const int chan = planar ? q >> 3 : b & 1;                 // chroma: 0 Cb, 1 Cr
            fill |= (uint32_t)((jb.fill >> (chroma ? 8 - 8 * chan : 16)) & 255) << (8 * e);
            if (i < t.ia || i >= t.ib || j < t.ja || j >= t.jb) inside &= ~(1u << e);
            else if (any < 0) any = col[e];
        }
        JM_SCL_UNROLL
        for (int e = 0; e < 4; e++) if (!((inside >> e) & 1)) col[e] = any < 0 ? 0 : any;     // a column the horizontal pass wrote
    }
    int o[4] = {0, 0, 0, 0};
    if (!PLACED || inside) vpass<4, PLACED>(t, i, hbuf, col, o);
    uint32_t v = 0;
    JM_SCL_UNROLL
    for (int e = 0; e < 4; e++) v |= (uint32_t)o[e] << (8 * e);
    if (PLACED && inside != 15) { uint32_t m = 0;
        JM_SCL_UNROLL
        for (int e = 0; e < 4; e++) if ((inside >> e) & 1) m |= 255u << (8 * e);
        v = (v & m) | (fill & ~m); }
    uint8_t *d;
    if (!chroma) d = jb.dst + (size_t)i * tw + t.j0 + 4 * q;
    else if (!planar) d = jb.dst + (size_t)tw * th + (size_t)i * tw + 2 * t.j0 + 4 * q;
    else d = jb.dst + (size_t)tw * th + (size_t)(q >> 3) * cw * ch + (size_t)i * cw + t.j0 + 4 * (q & 7);
    if (n_valid == 4 && !(((uintptr_t)d) & 3)) store_u32(d, v);
    else for (int e = 0; e < n_valid; e++) d[e] = (uint8_t)(v >> (8 * e));
}
JM_HD void vpass_store_lane(const ScaleJob &jb, const PlaneTile &t, int tid, const int16_t *hbuf) {
    if (t.placed) vpass_store_lane_t<true>(jb, t, tid, hbuf); else vpass_store_lane_t<false>(jb, t, tid, hbuf);
}

}  // namespace scl

// One axis of one plane's tap table: S source samples -> D outputs.  first[j] = first source index of output j (not clamped), w[j * taps + k] = weight
// of source index first[j] + k (1/16384; they sum to 16384).  Returns taps (the same for every output; unused taps weigh 0), or -1 when S, D are not
// positive or the ratio is outside 1/8 .. 4.  (Host: the tables are built when a geometry is activated.)
inline int build_scale_taps(int S, int D, std::vector<int32_t> &first, std::vector<int16_t> &w) {
    if (S <= 0 || D <= 0 || (long long)S > 8ll * D || (long long)D > 4ll * S) return -1;
    const long long s = S, d = D;
    int taps = 2;                                         // D >= S: bilinear, half-sample centres
    if (D < S) { taps = 0; for (long long j = 0; j < d; j++) { const int n = (int)(((j + 1) * s + d - 1) / d - j * s / d); if (n > taps) taps = n; } }    // area average
    first.assign((size_t)D, 0);
    w.assign((size_t)D * taps, 0);
    for (long long j = 0; j < d; j++) {
        int16_t *wj = &w[(size_t)j * taps];
        if (D >= S) {
            const long long num = (2 * j + 1) * s - d, d2 = 2 * d;
            const long long i0 = num >= 0 ? num / d2 : -((-num + d2 - 1) / d2);     // floor division
            const long long w1 = ((num - d2 * i0) * 16384 + d) / d2;
            first[j] = (int32_t)i0; wj[0] = (int16_t)(16384 - w1); wj[1] = (int16_t)w1;
        } else {
            const long long lo = j * s / d, hi = ((j + 1) * s + d - 1) / d;          // source samples lo .. hi - 1 overlap output j
            long long sum = 0, best = 0; int bk = 0;
            for (long long i = lo; i < hi; i++) {
                const long long a = ((i + 1) * d < (j + 1) * s ? (i + 1) * d : (j + 1) * s) - (i * d > j * s ? i * d : j * s);   // overlap; they sum to S
                wj[i - lo] = (int16_t)(a * 16384 / s); sum += wj[i - lo];
                if (a > best) { best = a; bk = (int)(i - lo); }
            }
            first[j] = (int32_t)lo; wj[bk] = (int16_t)(wj[bk] + 16384 - sum);      // the rounding remainder to the first largest overlap
        }
    }
    return taps;
}

}  // namespace jmamd
