// jmcodec_amd/csrc/mpeg2_recon.h -- the sample arithmetic of MPEG-2 decode (codec_type 4), INTEGRATION.md "MPEG-2": inverse quantisation, saturation
// and mismatch control (13818-2 7.4), the two IDCT passes of jpeg_recon.h, the prediction of 7.6 and the reconstruction, as __host__ __device__
// functions.  k_mpeg2_recon (mpeg2_kernels.hip) and the host reconstruction below run the same routines, so the CPU checks
// (tests/native/mpeg2_check.cpp, tools/fuzz_mpeg2.cpp) exercise the kernel's own arithmetic.  All int32, >> arithmetic, / truncating toward zero.
#pragma once
#include "jpeg_recon.h"
#include "mpeg2_jobs.h"

namespace jmamd {

// 7.4.2: F'' of one level at natural position pos, then 7.4.3 saturation.  intra DC: level * intra_dc_mult; intra AC: (2 QF W qs) / 32;
// non-intra: ((2 QF + sign(QF)) W qs) / 32.  |2 * 2047 + 1| * 255 * 112 < 1.2e8: inside int32
JR_HD int mpeg2_dequant(int level, int pos, bool intra, int w, int qs, int dc_mult) {
    int v;
    if (intra) v = pos == 0 ? level * dc_mult : (2 * level * w * qs) / 32;
    else v = level == 0 ? 0 : ((2 * level + (level > 0 ? 1 : -1)) * w * qs) / 32;
    return jpeg_clip(-2048, 2047, v);
}

// second IDCT pass, one row: r[x] = clip(-256, 255, (sum_u M[u][x] g[u] + 65536) >> 17)
JR_HD void mpeg2_pass2(const int g[8], int r[8]) {
JR_UNROLL
    for (int x = 0; x < 8; x++) {
        int a = 65536;
JR_UNROLL
        for (int u = 0; u < 8; u++) a += jpeg_m(u, x) * g[u];
        r[x] = jpeg_clip(-256, 255, a >> 17);
    }
}

// 7.6.4: one prediction sample of a plane (or of one field of it: base and pitch say which lines) at integer position (x, y) with the half-sample
// flags hx, hy; step 1 luma, 2 interleaved chroma.  Coordinates are clamped to [0, w - 1] x [0, h - 1]: no vector can make this read outside the plane
JR_HD int mpeg2_sample(const uint8_t *p, int pitch, int step, int x, int y, int hx, int hy, int w, int h) {
    const int x0 = jpeg_clip(0, w - 1, x), x1 = jpeg_clip(0, w - 1, x + hx), y0 = jpeg_clip(0, h - 1, y), y1 = jpeg_clip(0, h - 1, y + hy);
    const int a = p[(size_t)y0 * pitch + x0 * step];
    if (!hx && !hy) return a;
    if (hx && !hy) return (a + p[(size_t)y0 * pitch + x1 * step] + 1) >> 1;
    if (!hx) return (a + p[(size_t)y1 * pitch + x0 * step] + 1) >> 1;
    return (a + p[(size_t)y0 * pitch + x1 * step] + p[(size_t)y1 * pitch + x0 * step] + p[(size_t)y1 * pitch + x1 * step] + 2) >> 2;
}

// 7.6: the prediction of 8 neighbouring samples of plane row Y starting at X (frame coordinates of the plane), direction dir (0 forward, 1 backward).
// plane: the reference's luma (step 1) or one chroma component (step 2, chroma = true: the vector is the luma vector / 2 in both components);
// w x h: samples of the plane.  Field prediction (M2_FIELD_MV): line Y belongs to field Y & 1, predicted by vector Y & 1 from the field it selects
JR_HD void mpeg2_predict8(const Mpeg2Mb &mb, int dir, const uint8_t *plane, int pitch, int step, bool chroma, int w, int h, int X, int Y, int out[8]) {
    if (!plane) {
JR_UNROLL
        for (int j = 0; j < 8; j++) out[j] = 128;
        return;
    }
    const bool fld = (mb.flags & M2_FIELD_MV) != 0;
    const int r = fld ? (Y & 1) : 0;
    int mvx = mb.mv[dir * 2 + r][0], mvy = mb.mv[dir * 2 + r][1];
    if (chroma) { mvx /= 2; mvy /= 2; }
    const int hx = mvx & 1, hy = mvy & 1;
    if (fld) {
        const int sel = (mb.flags >> (M2_SEL_SHIFT + dir * 2 + r)) & 1;
        plane += (size_t)sel * pitch; pitch *= 2; Y >>= 1; h >>= 1;
    }
    const int x = X + (mvx >> 1), y = Y + (mvy >> 1);
JR_UNROLL
    for (int j = 0; j < 8; j++) out[j] = mpeg2_sample(plane, pitch, step, x + j, y, hx, hy, w, h);
}

// 7.6.7 + 7.6.8: 8 reconstructed samples from the residual r[] (already clipped to [-256, 255]; an uncoded block: zeros)
JR_HD void mpeg2_recon8(const Mpeg2Mb &mb, const uint8_t *const refp[2], int pitch, int step, bool chroma, int w, int h, int X, int Y, const int r[8],
                        uint8_t s[8]) {
    if (mb.flags & M2_INTRA) {
JR_UNROLL
        for (int j = 0; j < 8; j++) s[j] = (uint8_t)jpeg_clip(0, 255, r[j]);
        return;
    }
    int f[8], b[8];
    const bool fw = (mb.flags & M2_FWD) != 0, bw = (mb.flags & M2_BWD) != 0;
    if (fw) mpeg2_predict8(mb, 0, refp[0], pitch, step, chroma, w, h, X, Y, f);
    if (bw) mpeg2_predict8(mb, 1, refp[1], pitch, step, chroma, w, h, X, Y, b);
JR_UNROLL
    for (int j = 0; j < 8; j++) {
        const int p = fw && bw ? (f[j] + b[j] + 1) >> 1 : (fw ? f[j] : (bw ? b[j] : 0));
        s[j] = (uint8_t)jpeg_clip(0, 255, p + r[j]);
    }
}

// where block k (0..5) of a macroblock starts in the entry list, and how many entries it has; a record that points outside the list: an empty block
JR_HD int mpeg2_block_entries(const Mpeg2Mb &mb, int k, int n_entries, uint32_t *first) {
    uint32_t f = mb.first;
    for (int i = 0; i < k; i++) f += mb.count[i];
    int cnt = mb.count[k];
    if (cnt > 64 || (long long)f + cnt > (long long)n_entries) cnt = 0;
    *first = f;
    return cnt;
}

// one block on the host: entries -> 64 residuals in raster order (an empty block: zeros, no mismatch control -- the block was not coded)
inline void mpeg2_block_host(const Mpeg2PicParams &pp, const Mpeg2Mb &mb, int k, int res[64]) {
    int F[64] = {0}, g[64];
    uint32_t first; const int cnt = mpeg2_block_entries(mb, k, pp.n_entries, &first);
    const bool intra = (mb.flags & M2_INTRA) != 0;
    if (!cnt) { for (int i = 0; i < 64; i++) res[i] = 0; return; }
    for (int i = 0; i < cnt; i++) { const uint32_t e = pp.entries[first + i]; const int pos = (int)(e & 63);
        F[pos] = mpeg2_dequant((int)(int16_t)(e >> 16), pos, intra, pp.w[intra ? 0 : 1][pos], mb.qscale, pp.dc_mult); }
    int sum = 0; for (int i = 0; i < 64; i++) sum += F[i];
    if (!(sum & 1)) F[63] ^= 1;                                                    // 7.4.4 mismatch control
    for (int u = 0; u < 8; u++) { int col[8], o[8]; for (int v = 0; v < 8; v++) col[v] = F[v * 8 + u]; jpeg_pass1(col, o);
        for (int y = 0; y < 8; y++) g[y * 8 + u] = o[y]; }
    for (int y = 0; y < 8; y++) mpeg2_pass2(g + y * 8, res + y * 8);
}

// Host reconstruction of a whole picture from its job list into pp.surf (an NV12 surface like the device's; every pointer of pp is host memory)
inline void mpeg2_reconstruct_host(const Mpeg2PicParams &pp) {
    const int W = pp.mb_w * 16, H = pp.mb_h * 16;
    for (int my = 0; my < pp.mb_h; my++) for (int mx = 0; mx < pp.mb_w; mx++) {
        const Mpeg2Mb &mb = pp.mbs[(size_t)my * pp.mb_w + mx];
        int res[64]; uint8_t s[8];
        for (int k = 0; k < 4; k++) {
            mpeg2_block_host(pp, mb, k, res);
            for (int y = 0; y < 8; y++) {
                const int sr = (mb.flags & M2_FIELD_DCT) ? 2 * y + (k >> 1) : 8 * (k >> 1) + y;
                const int X = mx * 16 + (k & 1) * 8, Y = my * 16 + sr;
                mpeg2_recon8(mb, pp.ref, pp.pitch, 1, false, W, H, X, Y, res + y * 8, s);
                for (int j = 0; j < 8; j++) pp.surf[(size_t)Y * pp.pitch + X + j] = s[j];
            }
        }
        for (int c = 0; c < 2; c++) {
            mpeg2_block_host(pp, mb, 4 + c, res);
            const uint8_t *refc[2] = {pp.ref[0] ? pp.ref[0] + pp.chroma_offset + c : nullptr, pp.ref[1] ? pp.ref[1] + pp.chroma_offset + c : nullptr};
            for (int y = 0; y < 8; y++) {
                const int X = mx * 8, Y = my * 8 + y;
                mpeg2_recon8(mb, refc, pp.pitch, 2, true, W / 2, H / 2, X, Y, res + y * 8, s);
                for (int j = 0; j < 8; j++) pp.surf[pp.chroma_offset + (size_t)Y * pp.pitch + (X + j) * 2 + c] = s[j];
            }
        }
    }
}

}  // namespace jmamd
