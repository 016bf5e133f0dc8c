// jmcodec_amd/csrc/jpeg_kernels.hip -- k_jpeg_recon: MJPEG pictures (codec_type 2) from their sparse job lists into NV12 surfaces, gfx950.
//
// One wave per work item.  A luma item is 8 neighbouring blocks of one block row, a 64 x 8 strip; a chroma item is 4 Cb + 4 Cr blocks of the same
// positions, stored interleaved (4:2:0: 8 rows of 64 bytes; 4:2:2: the rows averaged in pairs, 4 rows of 64 bytes; 4:4:4: 2x2 cells averaged, 4 rows
// of 32 bytes).  The levels are scattered into zeroed LDS (dequantised on the way), the two IDCT passes run through LDS -- first pass: a lane per
// column, second pass: a lane per row -- and the lanes are dealt for the second pass so that lane l holds bytes 8 (l & 7) .. of strip row l >> 3:
// every store instruction writes whole 64-byte rows.  The arithmetic is jpeg_recon.h's, shared with the host checks.  No MFMA: a 1080p picture is 50 M
// integer multiply-adds; the kernel is bound by its list reads and 1.5 W H bytes of stores.
// LDS, by the bank rules of gfx950 (a 4-byte or narrower read and every write: bank = dword mod 32, serviced in 32-lane halves -- 16-lane quarters for
// an 8-byte write; a 16-byte read: bank = dword mod 64, in four fixed 16-lane groups).  The blocks of a strip are padded apart, because with the dense
// strides (32 / 64 / 16 dwords) every access below met the same banks in 4 blocks at once:
//   F  int16, 8 x 8 per block, block stride kFStride = 72 (36 dwords): the column read of pass 1 takes 4 dwords per block, 4 blocks per half at
//      dwords 0, 36, 72, 108 -- banks 0, 4, 8, 12: no conflict.  (The scatter's 2-byte writes go where the entries say.)
//   g  int32, row stride kGRow = 12, block stride kGStride = 112: the write of pass 1 puts 8 lanes of each of 4 blocks at banks 0, 16, 0, 16 (+ 12 y):
//      2-way, which a 4-byte write hides behind its own data transfer; the two 16-byte reads of pass 2 (lane = block l & 7, row l >> 3) take 16
//      distinct 4-bank slots in each of the four groups: no conflict.
//   s  bytes (chroma only), 8 x 8 per block, block stride kSStride = 80 (20 dwords): the 8-byte write and the byte reads of 4:2:0 without conflict,
//      the byte reads of 4:2:2 and 4:4:4 2-way.
// These counts are worked out from the addresses, not measured.  Every barrier is reached by every wave of the workgroup (inactive waves run with empty
// blocks and store nothing).
#include <hip/hip_runtime.h>
#include "jpeg_jobs.h"
#include "jpeg_recon.h"
#include "jpeg_entropy.h"

namespace jmamd {

constexpr int kJpegWaves = 4;
constexpr int kFStride = 72, kGRow = 12, kGStride = 112, kSStride = 80;

__global__ __launch_bounds__(64 * kJpegWaves) void k_jpeg_recon(const JpegPicParams *pics) {
    const JpegPicParams &pp = pics[blockIdx.y];
    if ((int)blockIdx.x * kJpegWaves >= pp.n_items) return;             // (the whole workgroup: no barrier is left behind)
    __shared__ __attribute__((aligned(16))) int16_t sF[kJpegWaves][8][kFStride];
    __shared__ __attribute__((aligned(16))) int sG[kJpegWaves][8][kGStride];
    __shared__ __attribute__((aligned(16))) uint8_t sS[kJpegWaves][8][kSStride];
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int item = (int)blockIdx.x * kJpegWaves + wave;
    const bool active = item < pp.n_items, luma = item < pp.n_items_y;
    const int b = l >> 3, i = l & 7;                                    // scatter and first pass: block b, entry lane / column i
    int row, sx, comp = 0; bool valid; size_t idx;
    if (luma) {
        const int spr = (pp.y_bw + 7) >> 3;
        row = item / spr; sx = item - row * spr;
        const int bx = sx * 8 + b;
        valid = active && bx < pp.y_bw; idx = (size_t)row * pp.y_bw + bx;
    } else {
        const int it = item - pp.n_items_y, spr = max(1, (pp.c_bw + 3) >> 2);        // (an inactive wave of a grey picture: no chroma strips at all)
        row = it / spr; sx = it - row * spr;
        const int bx = sx * 4 + (b >> 1);
        comp = 1 + (b & 1);
        valid = active && bx < pp.c_bw;
        idx = (size_t)pp.y_bw * pp.y_bh + (size_t)(b & 1) * pp.c_bw * pp.c_bh + (size_t)row * pp.c_bw + bx;
    }
    *reinterpret_cast<uint4 *>(&sF[wave][b][i * 8]) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    int cnt = 0; uint32_t first = 0;
    if (valid) { cnt = pp.count[idx]; first = pp.first[idx]; if (cnt > 64 || (long long)first + cnt > (long long)pp.n_entries) cnt = 0; }
    for (int e = i; e < cnt; e += 8) {
        const uint32_t v = pp.entries[first + e];
        const int k = (int)(v & 63);
        sF[wave][b][jpeg_zigzag(k)] = (int16_t)jpeg_dequant((int)(int16_t)(v >> 16), pp.q[comp][k]);
    }
    __syncthreads();
    {
        int F[8], g[8];
#pragma unroll
        for (int v = 0; v < 8; v++) F[v] = sF[wave][b][v * 8 + i];
        jpeg_pass1(F, g);
#pragma unroll
        for (int y = 0; y < 8; y++) sG[wave][b][y * kGRow + i] = g[y];
    }
    __syncthreads();
    const int bb = l & 7, y = l >> 3;                                   // second pass: row y of block bb
    uint2 px;
    {
        int g[8]; uint8_t s[8];
        const int4 g0 = *reinterpret_cast<const int4 *>(&sG[wave][bb][y * kGRow]), g1 = *reinterpret_cast<const int4 *>(&sG[wave][bb][y * kGRow + 4]);
        g[0] = g0.x; g[1] = g0.y; g[2] = g0.z; g[3] = g0.w; g[4] = g1.x; g[5] = g1.y; g[6] = g1.z; g[7] = g1.w;
        jpeg_pass2(g, s);
        px.x = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
        px.y = (uint32_t)s[4] | (uint32_t)s[5] << 8 | (uint32_t)s[6] << 16 | (uint32_t)s[7] << 24;
    }
    if (luma) {
        const int x0 = sx * 64 + bb * 8, Y = row * 8 + y;
        if (active && sx * 8 + bb < pp.y_bw && x0 + 8 <= pp.coded_w && Y < pp.coded_h)
            *reinterpret_cast<uint2 *>(pp.surf + (size_t)Y * pp.pitch + x0) = px;
    } else *reinterpret_cast<uint2 *>(&sS[wave][bb][y * 8]) = px;
    __syncthreads();
    if (luma || !active) return;
    // chroma: lane l writes bytes 8 (l & 7) .. of output row l >> 3 (4:4:4: bytes 8 (l & 3) .. of row l >> 2) -- Cb, Cr pairs of four positions
    const int mode = pp.sampling;
    const int r = mode == 0x11 ? l >> 2 : l >> 3, seg = mode == 0x11 ? l & 3 : l & 7;
    if (r >= (mode == 0x22 ? 8 : 4)) return;
    const int pi = mode == 0x11 ? seg : seg >> 1, xo = mode == 0x11 ? 0 : (seg & 1) * 4;
    uint32_t out[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const uint8_t *s = sS[wave][2 * pi + c];
            int v;
            if (mode == 0x22) v = s[r * 8 + xo + j];
            else if (mode == 0x21) v = jpeg_avg2(s[2 * r * 8 + xo + j], s[(2 * r + 1) * 8 + xo + j]);
            else v = jpeg_avg4(s[2 * r * 8 + 2 * j], s[2 * r * 8 + 2 * j + 1], s[(2 * r + 1) * 8 + 2 * j], s[(2 * r + 1) * 8 + 2 * j + 1]);
            out[j >> 1] |= (uint32_t)v << (16 * (j & 1) + 8 * c);
        }
    const int CY = row * (mode == 0x22 ? 8 : 4) + r, col = mode == 0x11 ? sx * 32 + seg * 8 : sx * 64 + seg * 8;
    if (sx * 4 + pi < pp.c_bw && col + 8 <= pp.coded_w && CY < pp.coded_h / 2)
        *reinterpret_cast<uint2 *>(pp.surf + pp.chroma_offset + (size_t)CY * pp.pitch + col) = make_uint2(out[0], out[1]);
}

void launch_jpeg_recon(const JpegPicParams *d_pics, int n, int max_items, hipStream_t st) {
    if (n <= 0 || max_items <= 0) return;
    hipLaunchKernelGGL(k_jpeg_recon, dim3((max_items + kJpegWaves - 1) / kJpegWaves, n), dim3(64 * kJpegWaves), 0, st, d_pics);
}

// k_jpeg_entropy: option jpeg_device_entropy -- the Huffman decode of the pictures' restart segments (jpeg_entropy.h has the routine, the layout
// of what it reads and the bounds of its loops).  blockIdx.y = picture, one lane per segment, 64 consecutive segments of a picture per wave, one
// wave per workgroup.  Every lane runs the same decode-one-symbol sequence on its own bit window, so lanes diverge only where their blocks begin
// and end, and where one of them meets damage.
// Tables: staged in LDS by the workgroup (6 x 1420 = 8520 bytes).  The decode of a lane is one chain of dependent steps -- window -> look[] ->
// shift -> window -- so the latency of the table read is paid once per symbol and nothing hides it but the other waves of the SIMD; an LDS read
// is several times shorter than a read that has to come from the vector cache, and 64 lanes index the table at unrelated places, which LDS serves
// by bank while the cache would serve it by line.  Staging costs 8.5 KB of coalesced reads per wave against some 6 KB of stream bytes per LANE
// (1080p, one MCU row per segment).  This is reasoning from the code; profiles/r19_mjpeg_device_entropy.txt has what was measured.
// The stream bytes are read as aligned dwords from global memory, a lane's own 64-byte line lasting it 16 refills; entries, first[] and count[]
// are plain vector stores.  The status words are raised with ordinary atomics on vector addresses, and only by a lane that met damage.
__global__ __launch_bounds__(64) void k_jpeg_entropy(const JpegEntropyParams *pics) {
    const JpegEntropyParams &pp = pics[blockIdx.y];
    if ((int)blockIdx.x * 64 >= pp.n_segs) return;                      // (the whole workgroup: no barrier is left behind)
    __shared__ __attribute__((aligned(16))) uint32_t sTab[6 * sizeof(JpegDevHuff) / 4];
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(pp.tab);
        for (int i = threadIdx.x; i < (int)(6 * sizeof(JpegDevHuff) / 4); i += 64) sTab[i] = src[i];
    }
    __syncthreads();
    const int seg = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (seg >= pp.n_segs) return;
    const JpegSegment sg = pp.segs[seg];
    const int damage = jpeg_entropy_segment(pp.geom, reinterpret_cast<const JpegDevHuff *>(sTab), sg, pp.bytes, pp.first, pp.count, pp.entries, nullptr);
    if (damage) { atomicAdd(pp.status, 1u); atomicOr(pp.status + 1, (uint32_t)damage); }
}

void launch_jpeg_entropy(const JpegEntropyParams *d_pics, int n, int max_segs, hipStream_t st) {
    if (n <= 0 || max_segs <= 0) return;
    hipLaunchKernelGGL(k_jpeg_entropy, dim3((max_segs + 63) / 64, n), dim3(64), 0, st, d_pics);
}

}  // namespace jmamd
