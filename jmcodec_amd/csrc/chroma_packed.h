// jmcodec_amd/csrc/chroma_packed.h -- interpolated chroma of the RGB output (option rgb_chroma, INTEGRATION.md "RGB output": C applied to the 4:4:4
// frame G'), once (k_rgb_pack444, out_kernels.hip).
//
// G'_Y is R_G's luma.  G'_Cb / G'_Cr are the chroma planes of the crop resampled straight to the full target, Sc = S / 2 source samples -> D outputs per
// axis, with the tap table of the axis shifted by the siting q of the stream's chroma_sample_loc_type (build_chroma_taps below).  The workgroup is
// k_rgb_pack's: 256 lanes per output tile of 64 x 16 pixels, lane tid owns row tid / 16 and columns 4 q .. 4 q + 3.  The tile's chroma goes through the
// resampler's own passes (scl::hpass_lane_t, scl::vpass) as two half tiles of 32 columns x (U, V), each with a row buffer of scl::kScaleTileW int16 per
// source row -- together the 64 columns x (U, V) a tile of 64 pixels needs; a lane's four pixels lie in one half.  Then every lane converts its 4
// pixels, each with a chroma pair of its own.  A placed job: the half tiles inherit the luma tile's share of the rectangle (the target of the chroma
// tables is the rectangle at full resolution, so the placement is the luma's, not shifted).
// __host__ __device__ like scale_packed.h / rgb_packed.h: tests/test_rgb_chroma_host.py walks whole frames through these routines on the CPU
// (tests/native/chroma_packed_check.cpp), tools/chroma_packed_asan.cpp runs them under AddressSanitizer / UBSan.
#pragma once
#include "rgb_packed.h"

namespace jmamd {
namespace chr {

// chroma source rows one tile of 16 output rows can reach: Sc <= 4 D, so 15 output rows of at most 4 source rows each + 1 (floor), + 5 taps - 1, + 1
// (the siting shift moves the window, it does not widen it: at most 65); with slack
constexpr int kChromaMaxRows = 68;
constexpr int kChromaMaxTaps = 5;
constexpr int kHalfCols = scl::kRgbTileW / 2;           // pixels of a half tile: 32 columns x (U, V) fill a row of the buffer

// the siting shifts of chroma_sample_loc_type 0..5 (H.264 Figure E-1 / HEVC Figure E.1), in quarters of a chroma sample: horizontally -1 = cosited with
// the even luma column, 0 = centred; vertically -1 top, 0 centre, +1 bottom
JM_HD int siting_qx(int loc) { return (loc & 1) ? 0 : -1; }
JM_HD int siting_qy(int loc) { return loc < 2 ? 0 : (loc < 4 ? -1 : 1); }

// The two half tiles (columns j0 .. j0 + 31 and j0 + 32 .. of the luma tile y) of a job's chroma; false: the rows do not fit the buffers (cannot
// happen within the validated ratios)
JM_HD bool chroma_tiles(const RgbJob &jb, const scl::PlaneTile &y, scl::PlaneTile c[2]) {
    const ScaleJob &sj = jb.s;
    for (int h = 0; h < 2; h++) {
        scl::PlaneTile &t = c[h];
        t = y;
        t.plane = sj.src + sj.chroma_offset; t.chroma = true;      // (hpass_lane_t: buffer column 2 * column + channel, source byte 2 * x + channel)
        t.ax = jb.cax[0]; t.ay = jb.cax[1];
        t.ox = sj.crop_x >> 1; t.oy = sj.crop_y >> 1;
        t.j0 = y.j0 + h * kHalfCols; t.jn = scl::imax(0, scl::imin(kHalfCols, y.jn - h * kHalfCols));
        if (t.placed) { t.ja = scl::imax(y.ja, t.j0); t.jb = scl::imin(y.jb, t.j0 + t.jn); if (t.ja >= t.jb) t.ja = t.jb = t.j0; }
        else { t.ja = t.j0; t.jb = t.j0 + t.jn; }
        if (y.nrows == 0 || y.ia >= y.ib) { t.r0 = 0; t.nrows = 0; continue; }             // fill only: neither table nor source is read
        const int Sy = t.ay.src_len;
        t.r0 = scl::clamp_to(t.ay.first[t.ia - t.dy], Sy);
        t.nrows = scl::clamp_to(t.ay.first[t.ib - 1 - t.dy] + t.ay.taps - 1, Sy) - t.r0 + 1;
        if (t.nrows > kChromaMaxRows) return false;
    }
    return true;
}

// Horizontal chroma pass of lane tid at full output width: both half tiles, hc = [2][kChromaMaxRows * scl::kScaleTileW]
JM_HD void hpass_chroma_lane(const scl::PlaneTile c[2], int tid, int16_t *hc) {
    JM_SCL_UNROLL
    for (int h = 0; h < 2; h++) {
        if (c[h].nrows == 0) continue;
        scl::hpass_lane(c[h], tid, hc + h * kChromaMaxRows * scl::kScaleTileW);
    }
}

// Vertical chroma pass of lane tid: the (Cb, Cr) pairs of its four pixels.  `inside` = rgbp::inside_mask of the lane (an unplaced job: 15); a pixel
// outside the rectangle keeps what U / V held, a lane without one reads nothing
JM_HD void vpass_chroma_lane(const scl::PlaneTile c[2], int tid, const int16_t *hc, uint32_t inside, int U[4], int V[4]) {
    const int r = tid >> 4, q = tid & 15, h = q >> 3;
    const scl::PlaneTile &t = c[0];                              // (the halves share the rows and the vertical table: only the buffer differs)
    if (!inside || t.nrows == 0) return;
    int any = 0;
    JM_SCL_UNROLL
    for (int e = 3; e >= 0; e--) if ((inside >> e) & 1) any = e;
    int col[8], o[8];
    JM_SCL_UNROLL
    for (int e = 0; e < 4; e++) {
        const int jj = 4 * (q & 7) + (((inside >> e) & 1) ? e : any);      // (a column the horizontal pass wrote)
        col[e] = 2 * jj; col[4 + e] = 2 * jj + 1;
    }
    scl::vpass<8>(t, t.i0 + r, hc + h * kChromaMaxRows * scl::kScaleTileW, col, o);
    JM_SCL_UNROLL
    for (int e = 0; e < 4; e++) if ((inside >> e) & 1) { U[e] = o[e]; V[e] = o[4 + e]; }
}

// rgbp::convert_store_masked with a chroma pair per pixel: C of the lane's 4 pixels (n of them valid), the fill where `inside` is clear
JM_HD void convert_store_444(const RgbJob &jb, const int Y[4], const int U[4], const int V[4], size_t px, int n, uint32_t inside) {
    const ScaleJob &sj = jb.s;
    uint32_t s[3][4];
    const int fR = ((jb.fill >> 16) & 255) << 14, fG = ((jb.fill >> 8) & 255) << 14, fB = (jb.fill & 255) << 14;
    const int fa[3] = {jb.bgr ? fB : fR, fG, jb.bgr ? fR : fB};
    JM_SCL_UNROLL
    for (int e = 0; e < 4; e++) {
        const int yv = jb.cy * (Y[e] - jb.yo), d = U[e] - 128, f = V[e] - 128;
        const int aR = yv + jb.crv * f, aG = yv - jb.cgu * d - jb.cgv * f, aB = yv + jb.cbu * d;
        const bool in = (inside >> e) & 1;
        const int a[3] = {in ? (jb.bgr ? aB : aR) : fa[0], in ? aG : fa[1], in ? (jb.bgr ? aR : aB) : fa[2]};          // storage positions
        JM_SCL_UNROLL
        for (int c = 0; c < 3; c++) {
            if (jb.dtype == RGB_U8) s[c][e] = rgbp::rgb_u8(a[c]);
            else {
                const float v = rgbp::rgb_f32(a[c], jb.k[c], jb.b[c]);
                s[c][e] = jb.dtype == RGB_F32 ? rgbp::f32_bits(v) : jb.dtype == RGB_F16 ? rgbp::f32_to_f16(v) : rgbp::f32_to_bf16(v);
            }
        }
    }
    const int sz = jb.dtype == RGB_U8 ? 1 : (jb.dtype == RGB_F32 ? 4 : 2);
    if (jb.planar) {
        const size_t P = (size_t)sj.tw * sj.th;
        JM_SCL_UNROLL
        for (int c = 0; c < 3; c++) rgbp::store4(sj.dst + (c * P + px) * sz, sz, s[c], n);
    } else {
        uint32_t v[12];
        JM_SCL_UNROLL
        for (int e = 0; e < 4; e++) for (int c = 0; c < 3; c++) v[3 * e + c] = s[c][e];
        uint8_t *d = sj.dst + 3 * px * sz;
        JM_SCL_UNROLL
        for (int g = 0; g < 3; g++) rgbp::store4(d + 4 * g * sz, sz, v + 4 * g, 3 * n - 4 * g);
    }
}

}  // namespace chr

// One axis of a chroma plane's tap table to the FULL target: Sc chroma samples -> D outputs with the siting shift q (-1, 0, +1 quarters of a chroma
// sample; INTEGRATION.md "RGB output" states the formulas), in build_scale_taps' layout.  q = 0 is build_scale_taps(Sc, D), tap for tap.  Returns the
// taps per output, or -1 when Sc, D are not positive, q is not one of the three or the ratio is outside Sc <= 4 D, D <= 8 Sc.
inline int build_chroma_taps(int Sc, int D, int q, std::vector<int32_t> &first, std::vector<int16_t> &w) {
    if (Sc <= 0 || D <= 0 || q < -1 || q > 1 || (long long)Sc > 4ll * D || (long long)D > 8ll * Sc) return -1;
    const long long s = Sc, d = D, d4 = 4 * d;
    auto fdiv = [](long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };      // floor division, b > 0
    auto lo_of = [&](long long j) { return fdiv(4 * j * s - q * d, d4); };
    auto hi_of = [&](long long j) { return -fdiv(-(4 * (j + 1) * s - q * d), d4); };                // ceil
    int taps = 2;
    if (D < Sc) { taps = 0; for (long long j = 0; j < d; j++) { const int n = (int)(hi_of(j) - lo_of(j)); if (n > taps) taps = n; } }
    first.assign((size_t)D, 0);
    w.assign((size_t)D * taps, 0);
    for (long long j = 0; j < d; j++) {
        int16_t *wj = &w[(size_t)j * taps];
        if (D >= Sc) {
            const long long num = 2 * (2 * j + 1) * s - (2 + q) * d, i0 = fdiv(num, d4);
            const long long w1 = ((num - d4 * i0) * 16384 + 2 * d) / d4;
            first[j] = (int32_t)i0; wj[0] = (int16_t)(16384 - w1); wj[1] = (int16_t)w1;
        } else {
            const long long lo = lo_of(j), hi = hi_of(j);
            long long sum = 0, best = 0; int bk = 0;
            for (long long k = lo; k < hi; k++) {
                const long long b = (4 * k + 4 + q) * d < 4 * (j + 1) * s ? (4 * k + 4 + q) * d : 4 * (j + 1) * s;
                const long long a0 = (4 * k + q) * d > 4 * j * s ? (4 * k + q) * d : 4 * j * s, a = b - a0;         // overlap; they sum to 4 Sc
                wj[k - lo] = (int16_t)(a * 16384 / (4 * s)); sum += wj[k - lo];
                if (a > best) { best = a; bk = (int)(k - lo); }
            }
            first[j] = (int32_t)lo; wj[bk] = (int16_t)(wj[bk] + 16384 - sum);
        }
    }
    return taps;
}

}  // namespace jmamd
