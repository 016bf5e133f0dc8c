// jmcodec_amd/csrc/mpeg2_kernels.hip -- k_mpeg2_recon: MPEG-2 pictures (codec_type 4) from their job lists into NV12 surfaces, gfx950.
// (k_mpeg2_vlc, which writes those lists on the device with option mpeg2_device_vlc, is at the end of the file with a header of its own.)
//
// One wave per work item; blockIdx.y = picture.  An item is four neighbouring macroblocks of one macroblock row: a 64 x 16 luma strip and a 64 x 8
// strip of interleaved chroma.  Its 24 blocks go through the IDCT in three rounds of eight: round 0 the blocks Y0 Y1 of the four macroblocks, round 1
// Y2 Y3, round 2 Cb Cr.  Per round:
//   scatter   lane l: block b = l >> 3 (macroblock b >> 1), entry lane i = l & 7.  The block's levels go into zeroed LDS, dequantised and saturated on
//             the way (mpeg2_dequant);
//   pass 1    lane l: column i of block b.  The eight lanes of a block add up their columns (three xor shuffles inside the group of eight) and the
//             lane of column 7 toggles the low bit of F[7][7] when the sum is even -- mismatch control, only for a block that has entries;
//   pass 2    lane l: row y = l >> 3 of block bb = l & 7, eight residuals.  The lane fetches the prediction of its eight samples straight from the
//             reference surfaces (byte rows at a stride of pitch, or 2 pitch for field prediction; every coordinate clamped to the picture, so no
//             record can make it read outside a surface), reconstructs and stores 8 bytes.  Luma: strip row 8 r + y (frame DCT) or 2 y + r (field
//             DCT, which only changes which strip rows a block's rows land on), bytes 8 bb ..: a store instruction writes eight 64-byte rows.  Chroma:
//             the lanes of Cb and Cr of one macroblock (bb ^ 1) swap halves with one xor shuffle, so that each writes 8 interleaved bytes: eight
//             64-byte rows again.
// The arithmetic is mpeg2_recon.h's, shared with the host checks.  No MFMA: a 1080p picture is 50 M integer multiply-adds.
// LDS, by the bank rules of gfx950 (a 4-byte or narrower read and every write: bank = dword mod 32, serviced in 32-lane halves; a 16-byte read: bank =
// dword mod 64, in four fixed 16-lane groups) -- the layout and the access patterns are those of k_jpeg_recon:
//   F  int16, 8 x 8 per block, block stride kFStride = 72 (36 dwords): the column read of pass 1 takes 4 dwords per block, 4 blocks per half at
//      dwords 0, 36, 72, 108 -- banks 0, 4, 8, 12: no conflict.  (The scatter's 2-byte writes go where the entries say; the zeroing is one 16-byte
//      write per lane at consecutive addresses.)
//   g  int32, row stride kGRow = 12, block stride kGStride = 112: the write of pass 1 puts 8 lanes of each of 4 blocks at banks 0, 16, 0, 16 (+ 12 y):
//      2-way, which a 4-byte write hides behind its own data transfer; the two 16-byte reads of pass 2 (lane = block l & 7, row l >> 3) take 16
//      distinct 4-bank slots in each of the four groups: no conflict.
// 4 waves x (8 x 72 x 2 + 8 x 112 x 4) = 18,944 bytes per workgroup.  These counts are worked out from the addresses, not measured.
// Every barrier is reached by every wave of the workgroup: the three rounds are unconditional, inactive waves and macroblocks beyond the row's end run
// with empty blocks and store nothing, and the only early return is taken by a whole workgroup before the first barrier.  No lane leaves before the
// last shuffle.
//
// Two instantiations, chosen per launch (launch_mpeg2_recon): k_mpeg2_recon<false> is the kernel frame pictures have always run -- a batch without a
// field picture and without a 16x8 or dual-prime record runs it, unchanged.  k_mpeg2_recon<true> (option mpeg2_field_pictures) adds:
//   field pictures   Mpeg2PicParams::structure 1 / 2: mb_h / 2 rows of strips (mb_h and n_items are the field's), every store goes to the lines of the
//                    field's parity -- base + (structure - 1) pitch, lines 2 pitch apart, luma and interleaved chroma alike -- and nothing of the
//                    other parity is written; the prediction reads the reference FIELDS of Mpeg2PicParams::fref (mpeg2_recon8x);
//   16x8, dual prime which vector a row uses, and the second fetch with the average of dual prime, in frame pictures too.
// A frame picture without such a record computes in <true> what it computes in <false> (mpeg2_recon8x hands it to mpeg2_recon8), so a mixed batch is
// exact.  The barrier argument above holds for both: structure and the modes only change addresses and what pass 2 fetches; no barrier and no
// shuffle sits inside a branch on them.  The LDS layout is the same.
// gfx950 compile (-Rpass-analysis=kernel-resource-usage), read from the compiler, not measured:
//   k_mpeg2_recon<false>  78 VGPRs, 85 SGPRs, 68 bytes of scratch per lane, 18,944 bytes of LDS, 6 waves per SIMD
//                         (the kernel before the split: 78 VGPRs, 84 SGPRs, 68 bytes of scratch, 6 waves)
//   k_mpeg2_recon<true>   90 VGPRs, 96 SGPRs, 68 bytes of scratch per lane, 18,944 bytes of LDS, 5 waves per SIMD
// The 68 bytes of scratch were there before the split.  Presumably they are the two macroblock records a lane holds (ms, mp), whose count[] and mv[]
// are indexed by values the compiler does not know; that has not been examined.
#include <hip/hip_runtime.h>
#include "mpeg2_jobs.h"
#include "mpeg2_recon.h"
#include "mpeg2_vlc.h"

namespace jmamd {

constexpr int kM2Waves = 4;
constexpr int kM2FStride = 72, kM2GRow = 12, kM2GStride = 112;

template <bool EXT> __global__ __launch_bounds__(64 * kM2Waves) void k_mpeg2_recon(const Mpeg2PicParams *pics) {
    const Mpeg2PicParams &pp = pics[blockIdx.y];
    if ((int)blockIdx.x * kM2Waves >= pp.n_items) return;              // (the whole workgroup: no barrier is left behind)
    __shared__ __attribute__((aligned(16))) int16_t sF[kM2Waves][8][kM2FStride];
    __shared__ __attribute__((aligned(16))) int sG[kM2Waves][8][kM2GStride];
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int item = (int)blockIdx.x * kM2Waves + wave;
    const bool active = item < pp.n_items;
    const int spr = (pp.mb_w + 3) >> 2;                                 // strips per macroblock row
    const int row = item / spr, mbx0 = (item - row * spr) * 4;
    const int W = pp.mb_w * 16, H = pp.mb_h * 16;                      // (a field picture: mb_h and H are the field's)
    // EXT: a field picture stores the lines of its parity only -- from line structure - 1 on, 2 pitch apart
    const int structure = EXT ? pp.structure : 0;
    const int sp = structure ? 2 * pp.pitch : pp.pitch;
    uint8_t *const surf = pp.surf + (structure ? (size_t)(structure - 1) * pp.pitch : 0);
    const int b = l >> 3, i = l & 7;                                    // scatter and pass 1: block b, entry lane / column i
    const int bb = l & 7, y = l >> 3;                                   // pass 2: row y of block bb
    // the macroblock whose blocks this lane scatters (ms) and the one whose samples it reconstructs (mp)
    Mpeg2Mb ms = {}, mp = {};
    const bool valid_s = active && mbx0 + (b >> 1) < pp.mb_w, valid_p = active && mbx0 + (bb >> 1) < pp.mb_w;
    if (valid_s) ms = pp.mbs[(size_t)row * pp.mb_w + mbx0 + (b >> 1)];
    if (valid_p) mp = pp.mbs[(size_t)row * pp.mb_w + mbx0 + (bb >> 1)];
    const bool intra_s = (ms.flags & M2_INTRA) != 0;
    const uint8_t *wq = pp.w[intra_s ? 0 : 1];
#pragma unroll 1
    for (int r = 0; r < 3; r++) {
        *reinterpret_cast<uint4 *>(&sF[wave][b][i * 8]) = make_uint4(0, 0, 0, 0);
        __syncthreads();
        const int k = r < 2 ? 2 * r + (b & 1) : 4 + (b & 1);
        uint32_t first = 0;
        const int cnt = valid_s ? mpeg2_block_entries(ms, k, pp.n_entries, &first) : 0;
        for (int e = i; e < cnt; e += 8) {
            const uint32_t v = pp.entries[first + e];
            const int pos = (int)(v & 63);
            sF[wave][b][pos] = (int16_t)mpeg2_dequant((int)(int16_t)(v >> 16), pos, intra_s, wq[pos], ms.qscale, pp.dc_mult);
        }
        __syncthreads();
        {
            int F[8], g[8], sum = 0;
#pragma unroll
            for (int v = 0; v < 8; v++) { F[v] = sF[wave][b][v * 8 + i]; sum += F[v]; }
            sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4);
            if (cnt > 0 && i == 7 && !(sum & 1)) F[7] ^= 1;
            jpeg_pass1(F, g);
#pragma unroll
            for (int yy = 0; yy < 8; yy++) sG[wave][b][yy * kM2GRow + i] = g[yy];
        }
        __syncthreads();
        int res[8]; uint8_t s[8];
        {
            int g[8];
            const int4 g0 = *reinterpret_cast<const int4 *>(&sG[wave][bb][y * kM2GRow]), g1 = *reinterpret_cast<const int4 *>(&sG[wave][bb][y * kM2GRow + 4]);
            g[0] = g0.x; g[1] = g0.y; g[2] = g0.z; g[3] = g0.w; g[4] = g1.x; g[5] = g1.y; g[6] = g1.z; g[7] = g1.w;
            mpeg2_pass2(g, res);
        }
        if (r < 2) {
            const int sr = (mp.flags & M2_FIELD_DCT) ? 2 * y + r : 8 * r + y;
            const int X = (mbx0 + (bb >> 1)) * 16 + (bb & 1) * 8, Y = row * 16 + sr;
            if (valid_p) {
                if (EXT) { const uint8_t *fld[2][2]; mpeg2_ref_fields(pp, 0, fld); mpeg2_recon8x(mp, fld, pp.pitch, 1, false, W, H, X, Y, structure, res, s); }
                else mpeg2_recon8(mp, pp.ref, pp.pitch, 1, false, W, H, X, Y, res, s);
                uint2 px;
                px.x = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
                px.y = (uint32_t)s[4] | (uint32_t)s[5] << 8 | (uint32_t)s[6] << 16 | (uint32_t)s[7] << 24;
                if (X + 8 <= W && Y < H) *reinterpret_cast<uint2 *>(surf + (size_t)Y * sp + X) = px;
            }
        } else {
            const int c = bb & 1, X = (mbx0 + (bb >> 1)) * 8, Y = row * 8 + y;
            s[0] = s[1] = s[2] = s[3] = s[4] = s[5] = s[6] = s[7] = 0;
            if (valid_p) {
                if (EXT) { const uint8_t *fld[2][2]; mpeg2_ref_fields(pp, pp.chroma_offset + c, fld); mpeg2_recon8x(mp, fld, pp.pitch, 2, true, W >> 1, H >> 1, X, Y, structure, res, s); }
                else {
                    const uint8_t *refc[2] = {pp.ref[0] ? pp.ref[0] + pp.chroma_offset + c : nullptr, pp.ref[1] ? pp.ref[1] + pp.chroma_offset + c : nullptr};
                    mpeg2_recon8(mp, refc, pp.pitch, 2, true, W >> 1, H >> 1, X, Y, res, s);
                }
            }
            // the Cb lane keeps samples 0..3 and gets Cr's 0..3; the Cr lane keeps 4..7 and gets Cb's 4..7
            const uint32_t lo = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
            const uint32_t hi = (uint32_t)s[4] | (uint32_t)s[5] << 8 | (uint32_t)s[6] << 16 | (uint32_t)s[7] << 24;
            const uint32_t got = (uint32_t)__shfl_xor((int)(c ? lo : hi), 1);
            const uint32_t cb = c ? got : lo, cr = c ? hi : got;      // four Cb and four Cr samples of the same positions
            uint2 px;
            px.x = (cb & 0xff) | (cr & 0xff) << 8 | (cb & 0xff00) << 8 | (cr & 0xff00) << 16;
            px.y = (cb >> 16 & 0xff) | (cr >> 16 & 0xff) << 8 | (cb >> 24) << 16 | (cr >> 24) << 24;
            if (valid_p && 2 * X + 16 <= W && Y < (H >> 1))
                *reinterpret_cast<uint2 *>(surf + pp.chroma_offset + (size_t)Y * sp + 2 * X + c * 8) = px;
        }
        __syncthreads();                                                // (sG is read above and written by the next round's pass 1)
    }
}

void launch_mpeg2_recon(const Mpeg2PicParams *d_pics, int n, int max_items, bool ext, ihipStream_t *st) {
    if (n <= 0 || max_items <= 0) return;
    const dim3 grid((max_items + kM2Waves - 1) / kM2Waves, n), block(64 * kM2Waves);
    if (ext) hipLaunchKernelGGL(k_mpeg2_recon<true>, grid, block, 0, st, d_pics);
    else hipLaunchKernelGGL(k_mpeg2_recon<false>, grid, block, 0, st, d_pics);
}

// k_mpeg2_vlc: option mpeg2_device_vlc -- the slice / macroblock / block VLC decode of the pictures' slices (mpeg2_vlc.h has the routine, the layout of
// what it reads, the capacity and the bounds of its loops).  blockIdx.y = picture, one lane per slice, 64 consecutive slices of a picture per wave, one
// wave per workgroup: a wave holds slices of one picture only, so the picture's parameters are wave-uniform (they are read through a uniform
// pointer and stay in scalar registers).
// Tables: Mpeg2VlcTables, 15,936 bytes, staged in LDS by the workgroup with 16-byte copies -- 10 workgroups fit the 160 KiB of a CU by LDS.  One
// barrier follows the copy and every lane of the workgroup reaches it: the only return in front of it is taken by a whole workgroup, lanes beyond
// the picture's slice count idle behind it.
// A lane's decode is one chain of dependent steps -- window -> table -> shift -> window -- and 64 lanes are at unrelated places of the syntax
// (address increment, vectors, coefficients), so the wave runs the union of their branches: divergent and latency-bound, like k_jpeg_entropy; the
// table reads are LDS reads at unrelated addresses.  This is reasoning from the code; profiles/r20_mpeg2_device_vlc.txt has what was measured, and
// no bound is claimed beyond it.
// The slice bytes are read as aligned dwords from global memory (a lane's 64-byte line lasts it 16 refills); a record is two 16-byte vector
// stores, an entry one 4-byte store -- global_load / global_store: the routine casts the three arrays to global-memory pointers, as flat
// instructions would tie every table read's wait to the stores in flight -- and the status words are raised with ordinary atomics on vector addresses.  Plain C++, no inline assembly.
// The predictors (pmv, dc_pred) are indexed by constants only and live in registers.
// gfx950 compile (-Rpass-analysis=kernel-resource-usage): 129 VGPRs, 106 SGPRs (48 spilled to vector lanes), no scratch,
// 15,936 bytes of LDS, 3 waves per SIMD by the compiler's count (before the lane learned dual prime: 121 VGPRs, 42 spilled, 3 waves).
__global__ __launch_bounds__(64) void k_mpeg2_vlc(const Mpeg2VlcParams *pics) {
    const Mpeg2VlcParams &pp = pics[blockIdx.y];
    if ((int)blockIdx.x * 64 >= pp.n_slices) return;                    // (the whole workgroup: no barrier is left behind)
    __shared__ __attribute__((aligned(16))) uint4 sTab[sizeof(Mpeg2VlcTables) / 16];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(pp.tab);
        for (int i = threadIdx.x; i < (int)(sizeof(Mpeg2VlcTables) / 16); i += 64) sTab[i] = src[i];
    }
    __syncthreads();
    const int s = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (s >= pp.n_slices) return;
    const Mpeg2VlcPic pic = *pp.pic;
    const Mpeg2Slice sl = pp.slices[s];
    uint32_t n_dual = 0;
    const uint32_t st = mpeg2_vlc_slice(pic, reinterpret_cast<const Mpeg2VlcTables *>(sTab), sl, pp.bytes, pp.mbs, pp.entries, nullptr, &n_dual);
    if (n_dual) atomicAdd(pp.status + 3, n_dual << 8);                  // (bits 8.. of the flag word count the dual-prime records; the flags are ORed into bits 0 and 1)
    if (st & kM2StKindMask) { atomicAdd(pp.status, 1u); atomicOr(pp.status + 1, 1u << (st & kM2StKindMask)); }
    if (st >> kM2StClampedShift) atomicAdd(pp.status + 2, st >> kM2StClampedShift);
    if (st & (kM2StHoles | kM2StDualPrime)) atomicOr(pp.status + 3, ((st & kM2StHoles) ? 1u : 0u) | ((st & kM2StDualPrime) ? 2u : 0u));
}

void launch_mpeg2_vlc(const Mpeg2VlcParams *d_pics, int n, int max_slices, ihipStream_t *st) {
    if (n <= 0 || max_slices <= 0) return;
    hipLaunchKernelGGL(k_mpeg2_vlc, dim3((max_slices + 63) / 64, n), dim3(64), 0, st, d_pics);
}

}  // namespace jmamd
