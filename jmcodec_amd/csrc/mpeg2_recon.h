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

// ---- option mpeg2_field_pictures: field pictures, 16x8 motion compensation and dual prime (7.6.2.1, 7.6.3.6, 7.6.4) ----
// 8 prediction samples from ONE field: fld = the first sample of the field's plane (nullptr: 128), its lines pitch2 apart, w x hf samples;
// (X, Yf): position in that field; the vector is the luma vector in half samples, y in lines of the field (chroma halves it, truncating)
JR_HD void mpeg2_fetch8(const uint8_t *fld, int pitch2, int step, bool chroma, int w, int hf, int X, int Yf, int mvx, int mvy, int out[8]) {
    if (!fld) {
JR_UNROLL
        for (int j = 0; j < 8; j++) out[j] = 128;
        return;
    }
    if (chroma) { mvx /= 2; mvy /= 2; }
    const int hx = mvx & 1, hy = mvy & 1, x = X + (mvx >> 1), y = Yf + (mvy >> 1);
JR_UNROLL
    for (int j = 0; j < 8; j++) out[j] = mpeg2_sample(fld, pitch2, step, x + j, y, hx, hy, w, hf);
}

// mpeg2_recon8 for every mode of mpeg2_jobs.h.  fld[direction][parity]: the first sample of each reference field's plane (luma, or one chroma
// component), lines 2 pitch apart -- a frame picture passes its reference frame's two fields.  structure: Mpeg2PicParams::structure.  Frame picture:
// (X, Y) and w x h are the frame's, as for mpeg2_recon8; field picture: (X, Y) is the position in the field and h the FIELD's height.
JR_HD void mpeg2_recon8x(const Mpeg2Mb &mb, const uint8_t *const fld[2][2], int pitch, int step, bool chroma, int w, int h, int X, int Y, int structure,
                         const int r[8], uint8_t s[8]) {
    if (!structure && !(mb.flags & M2_DUAL)) {             // (a frame's plane starts where its top field does)
        const uint8_t *const refp[2] = {fld[0][0], fld[1][0]};
        mpeg2_recon8(mb, refp, pitch, step, chroma, w, h, X, Y, r, s);
        return;
    }
    if (mb.flags & M2_INTRA) {
JR_UNROLL
        for (int j = 0; j < 8; j++) s[j] = (uint8_t)jpeg_clip(0, 255, r[j]);
        return;
    }
    int f[8], b[8];
    bool two;
    if (mb.flags & M2_DUAL) {
        // same parity with the transmitted vector, opposite parity with the derived one
        const int par = structure ? structure - 1 : (Y & 1), Yf = structure ? Y : Y >> 1, hf = structure ? h : h >> 1;
        const int d = structure ? 2 : 2 + par;
        mpeg2_fetch8(fld[0][par], 2 * pitch, step, chroma, w, hf, X, Yf, mb.mv[0][0], mb.mv[0][1], f);
        mpeg2_fetch8(fld[0][par ^ 1], 2 * pitch, step, chroma, w, hf, X, Yf, mb.mv[d][0], mb.mv[d][1], b);
        two = true;
    } else {
        const int v = (mb.flags & M2_16X8) ? (Y >> (chroma ? 2 : 3)) & 1 : 0;
        const bool fw = (mb.flags & M2_FWD) != 0, bw = (mb.flags & M2_BWD) != 0;
        if (fw) mpeg2_fetch8(fld[0][(mb.flags >> (M2_SEL_SHIFT + v)) & 1], 2 * pitch, step, chroma, w, h, X, Y, mb.mv[v][0], mb.mv[v][1], f);
        if (bw) mpeg2_fetch8(fld[1][(mb.flags >> (M2_SEL_SHIFT + 2 + v)) & 1], 2 * pitch, step, chroma, w, h, X, Y, mb.mv[2 + v][0], mb.mv[2 + v][1], fw ? b : f);
        if (!fw && !bw) {
JR_UNROLL
            for (int j = 0; j < 8; j++) f[j] = 0;
        }
        two = fw && bw;
    }
JR_UNROLL
    for (int j = 0; j < 8; j++) s[j] = (uint8_t)jpeg_clip(0, 255, (two ? (f[j] + b[j] + 1) >> 1 : f[j]) + r[j]);
}

// the fields of a picture's references as mpeg2_recon8x wants them: off = 0 for luma, chroma_offset + c for a chroma component
JR_HD void mpeg2_ref_fields(const Mpeg2PicParams &pp, int off, const uint8_t *fld[2][2]) {
JR_UNROLL
    for (int d = 0; d < 2; d++)
JR_UNROLL
        for (int p = 0; p < 2; p++) {
            const uint8_t *q = pp.structure ? pp.fref[d][p] : (pp.ref[d] ? pp.ref[d] + (size_t)p * pp.pitch : nullptr);
            fld[d][p] = q ? q + off : nullptr;
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

// Host reconstruction of a whole picture from its job list into pp.surf (an NV12 surface like the device's; every pointer of pp is host memory).
// A field picture (pp.structure) stores the lines of its parity only.  Like the device, it runs mpeg2_recon8 unless the picture says `ext`
inline void mpeg2_reconstruct_host(const Mpeg2PicParams &pp) {
    const int W = pp.mb_w * 16, H = pp.mb_h * 16;
    const bool ext = pp.ext || pp.structure;
    const int sp = pp.structure ? 2 * pp.pitch : pp.pitch;                          // the pitch of the lines that are stored
    uint8_t *const surf = pp.surf + (pp.structure ? (size_t)(pp.structure - 1) * pp.pitch : 0);
    const uint8_t *fy[2][2], *fc[2][2];
    mpeg2_ref_fields(pp, 0, fy);
    for (int my = 0; my < pp.mb_h; my++) for (int mx = 0; mx < pp.mb_w; mx++) {
        const Mpeg2Mb &mb = pp.mbs[(size_t)my * pp.mb_w + mx];
        int res[64]; uint8_t s[8];
        for (int k = 0; k < 4; k++) {
            mpeg2_block_host(pp, mb, k, res);
            for (int y = 0; y < 8; y++) {
                const int sr = (mb.flags & M2_FIELD_DCT) ? 2 * y + (k >> 1) : 8 * (k >> 1) + y;
                const int X = mx * 16 + (k & 1) * 8, Y = my * 16 + sr;
                if (ext) mpeg2_recon8x(mb, fy, pp.pitch, 1, false, W, H, X, Y, pp.structure, res + y * 8, s);
                else mpeg2_recon8(mb, pp.ref, pp.pitch, 1, false, W, H, X, Y, res + y * 8, s);
                for (int j = 0; j < 8; j++) surf[(size_t)Y * sp + X + j] = s[j];
            }
        }
        for (int c = 0; c < 2; c++) {
            mpeg2_block_host(pp, mb, 4 + c, res);
            const uint8_t *refc[2] = {pp.ref[0] ? pp.ref[0] + pp.chroma_offset + c : nullptr, pp.ref[1] ? pp.ref[1] + pp.chroma_offset + c : nullptr};
            mpeg2_ref_fields(pp, pp.chroma_offset + c, fc);
            for (int y = 0; y < 8; y++) {
                const int X = mx * 8, Y = my * 8 + y;
                if (ext) mpeg2_recon8x(mb, fc, pp.pitch, 2, true, W / 2, H / 2, X, Y, pp.structure, res + y * 8, s);
                else mpeg2_recon8(mb, refc, pp.pitch, 2, true, W / 2, H / 2, X, Y, res + y * 8, s);
                for (int j = 0; j < 8; j++) surf[pp.chroma_offset + (size_t)Y * sp + (X + j) * 2 + c] = s[j];
            }
        }
    }
}

}  // namespace jmamd
