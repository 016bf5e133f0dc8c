// jmcodec_amd/csrc/jpeg_entropy.h -- MJPEG (codec_type 2), option jpeg_device_entropy: the Huffman decode of one restart segment as a
// __host__ __device__ routine.  k_jpeg_entropy (jpeg_kernels.hip) runs it with one lane per segment; tests/native/jpeg_entropy_check.cpp and
// tools/jpeg_entropy_asan.cpp walk the same code on the CPU.  No HIP header: g++ builds it.
//
// What the device is given (built by jpeg_segment_scan, jpeg_syntax.cpp; layout of the uploaded blob: INTEGRATION.md "MJPEG"):
//   tables    JpegDevHuff[6]: the DC tables of components 0..2, then the AC tables -- look / maxcode / valoff / vals of JpegHuff, 1420 bytes each;
//   segments  JpegSegment[n]: where the segment's clean bytes start, how many there are, the MCUs it covers, where its entries go and how many fit;
//   bytes     per segment the entropy-coded bytes between two markers with FF 00 unstuffed to FF, fill bytes and the RSTn marker removed, padded
//             with zeros to a multiple of 4 and followed by kJpegSegGuard zero bytes.  Every segment starts at a multiple of 4, so the reader
//             takes whole aligned dwords; a marker never has to be recognised here, and bytes behind the segment read as zeros, which is what
//             jpeg_decode_scan's reader supplies behind a marker.
// The guard: a symbol is at most 16 code bits + 15 value bits, read from a 64-bit window that is topped up one dword at a time whenever it holds 32
// bits or fewer.  Decoding stops at the first symbol that ends beyond bit 8 L, so no bit beyond 8 L + 31 is ever used and no dword beyond byte
// L + 12 is fetched: pad4(L) + 16 bytes cover it.  The reader checks its dword index against that size all the same and supplies zeros beyond it.
//
// Entry capacity of a segment of L bytes and B blocks: min(64 B, 4 L + B).
//   An AC entry takes a Huffman code of at least 1 bit and s >= 1 value bits; a DC entry whose difference is non-zero likewise: 2 bits or more.
//   Only a DC entry with s = 0 (the predictor stays at a non-zero value) costs as little as 1 bit, and a block has one DC symbol.  With E2 entries
//   of the first kind and E1 <= B of the second, 2 E2 + E1 <= 8 L, so E1 + E2 <= 4 L + B; 64 per block bounds it too.  (The first block of a
//   segment starts from predictor 0, so its DC entry is never of the cheap kind and 4 L + B - 1 would do; the tests reach min(64 B, 4 L + B) where
//   64 B is the smaller: one block of 64 two-bit entries in 16 bytes.)  An entry is written only after the symbol that produced it was found to
//   end inside the segment, so the bound holds for damaged segments as well; the routine checks every write against the capacity anyway and
//   treats an overflow as damage.
//
// Loops: the symbol loop decodes one Huffman symbol per iteration, which consumes at least one bit and moves k forward by at least one (the DC
// symbol from 0 to 1), so it runs at most min(8 L + 1, 64 B) times; the loop that empties the blocks behind damage runs at most B times.  Both
// together stay below 8 L + 65 B iterations -- the for-loops carry 64 B and B as their limits, and the CPU walk asserts the count.
//
// Damage: an invalid code, a DC category above 15, a run that passes position 63, a symbol that ends beyond bit 8 L, an entry beyond the capacity.
// The block that met it and every later block of the SEGMENT get count 0; other segments are not affected.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JE_HD __host__ __device__ __forceinline__
#else
#define JE_HD inline
#endif

namespace jmamd {

constexpr int kJpegSegGuard = 16;          // zero bytes behind every segment's padded bytes

struct JpegDevHuff {                       // JpegHuff without bits[] (jpeg_syntax.h)
    uint16_t look[512];                    // by the next 9 bits: length << 8 | symbol (0: longer than 9 bits, or no such code)
    int32_t maxcode[18], valoff[17];
    uint8_t vals[256];
};
static_assert(sizeof(JpegDevHuff) == 1420, "the device form of a Huffman table is 1420 bytes");

struct JpegSegment {
    uint32_t byte_off;                     // of its clean bytes, from the start of the picture's clean bytes; a multiple of 4
    uint32_t n_bytes;                      // L: exact length (0: an empty segment -- its restart marker was missing)
    uint32_t first_mcu, n_mcus;
    uint32_t first_entry, entry_cap;       // its entries go to entries[first_entry .. first_entry + entry_cap)
};

struct JpegScanGeom {                      // of JpegPic: what maps (MCU, block in MCU) to a block index in plane raster order
    int ncomp, hs, vs, mcus_x;
    int y_bw, y_bh, c_bw, c_bh;
};

JE_HD uint32_t jpeg_entropy_capacity(uint32_t n_bytes, uint32_t n_blocks) {
    const uint64_t a = 64ull * n_blocks, b = 4ull * n_bytes + n_blocks;
    return (uint32_t)(a < b ? a : b);
}
// bytes a segment of L bytes takes in the clean byte array
JE_HD uint32_t jpeg_entropy_padded(uint32_t n_bytes) { return ((n_bytes + 3u) & ~3u) + (uint32_t)kJpegSegGuard; }

constexpr int kJpegDamageCode = 1, kJpegDamageEnd = 2, kJpegDamageCap = 4;

// block `b` of MCU `mcu` (scan order) -> its index in plane raster order (the indexing of jpeg_decode_scan) and its component
JE_HD uint32_t jpeg_entropy_block_index(const JpegScanGeom &g, uint32_t mcu, int b, int *comp) {
    const uint32_t my = mcu / (uint32_t)g.mcus_x, mx = mcu % (uint32_t)g.mcus_x;
    const int ny = g.hs * g.vs;
    if (b < ny || g.ncomp == 1) { *comp = 0; return (my * (uint32_t)g.vs + (uint32_t)(b / g.hs)) * (uint32_t)g.y_bw + mx * (uint32_t)g.hs + (uint32_t)(b % g.hs); }
    const int c = b - ny + 1; *comp = c;
    return (uint32_t)g.y_bw * (uint32_t)g.y_bh + (uint32_t)(c - 1) * (uint32_t)g.c_bw * (uint32_t)g.c_bh + my * (uint32_t)g.c_bw + mx;
}

// Decodes segment sg.  tab: the six tables; bytes: the picture's clean bytes (4-byte aligned).  Writes first[] / count[] of every block of the
// segment and its entries; returns 0, or the kind of damage (kJpegDamage*).  *iters (may be null) receives the number of loop iterations.
JE_HD int jpeg_entropy_segment(const JpegScanGeom &g, const JpegDevHuff *tab, const JpegSegment &sg, const uint32_t *bytes,
                               uint32_t *first, uint8_t *count, uint32_t *entries, long long *iters) {
    const int bpm = g.ncomp == 3 ? g.hs * g.vs + 2 : 1;
    const uint32_t n_blocks = sg.n_mcus * (uint32_t)bpm;
    const uint32_t *w = bytes + (sg.byte_off >> 2);
    const uint32_t n_words = jpeg_entropy_padded(sg.n_bytes) >> 2;
    const long long end_bit = 8ll * sg.n_bytes;
    const uint32_t e_end = sg.first_entry + sg.entry_cap;
    uint64_t acc = 0; int n = 0; uint32_t wi = 0;                // the window: n valid bits at the top of acc; wi dwords fetched so far
    long long p0 = 0, p1 = 0, p2 = 0;                           // DC predictors: 64 bits, as on the host (a whole picture may be one segment)
    uint32_t e = sg.first_entry, blk = 0, idx = 0, blk_first = e;
    int k = 0, c = 0, damage = 0;
    long long it = 0;
    const long long limit = 64ll * n_blocks;
    for (; it < limit && blk < n_blocks; it++) {
        if (n <= 32) { const uint32_t v = wi < n_words ? __builtin_bswap32(w[wi]) : 0u; acc |= (uint64_t)v << (32 - n); n += 32; wi++; }
        if (k == 0) {                                           // a block begins: where its record goes
            idx = jpeg_entropy_block_index(g, sg.first_mcu + blk / (uint32_t)bpm, (int)(blk % (uint32_t)bpm), &c);
            blk_first = e;
            first[idx] = e;
        }
        // one Huffman symbol of the component's DC or AC table (at least 1 bit)
        const JpegDevHuff &h = tab[(k == 0 ? 0 : 3) + c];
        int sym = -1, len = 0;
        const unsigned look = h.look[(unsigned)(acc >> 55)];
        if (look) { len = (int)(look >> 8); sym = (int)(look & 255); }
        else {
            const unsigned c16 = (unsigned)(acc >> 48);
            for (int l = 16; l >= 10; l--) { const int cd = (int)(c16 >> (16 - l)); if (cd <= h.maxcode[l]) { len = l; sym = h.vals[(h.valoff[l] + cd) & 255]; } }
        }
        if (sym < 0 || (k == 0 && sym > 15)) { damage = kJpegDamageCode; break; }
        acc <<= len; n -= len;
        // its value bits: the DC category, or the low nibble of an AC symbol
        const int s = k == 0 ? sym : (sym & 15), run = k == 0 ? 0 : (sym >> 4);
        int v = 0;
        if (s) { v = (int)(acc >> (64 - s)); acc <<= s; n -= s; if (v < (1 << (s - 1))) v -= (1 << s) - 1; }
        if (32ll * (long long)wi - n > end_bit) { damage = kJpegDamageEnd; break; }      // the symbol ends beyond the segment's last bit
        long long level = v; int pos = 0; bool put = s != 0;
        if (k == 0) {
            if (c == 0) level = (p0 += v); else if (c == 1) level = (p1 += v); else level = (p2 += v);
            put = level != 0; k = 1;
        } else if (s == 0) k = run == 15 ? k + 16 : 64;         // ZRL; EOB
        else {
            k += run;
            if (k > 63) { damage = kJpegDamageCode; break; }
            pos = k++;
        }
        if (put) {
            if (e >= e_end) { damage = kJpegDamageCap; break; }
            const int lv = level < -32768 ? -32768 : (level > 32767 ? 32767 : (int)level);       // (leaves clip(level * Q) unchanged: jpeg_jobs.h)
            entries[e++] = (uint32_t)pos | (uint32_t)(uint16_t)lv << 16;
        }
        if (k >= 64) { count[idx] = (uint8_t)(e - blk_first); blk++; k = 0; }
    }
    if (!damage && blk < n_blocks) damage = kJpegDamageCode;    // (not reachable: k moves forward in every iteration)
    // behind damage: the block that met it and every later block of the segment are empty
    for (long long j = 0; damage && j < (long long)n_blocks && blk < n_blocks; j++, blk++, it++) {
        idx = jpeg_entropy_block_index(g, sg.first_mcu + blk / (uint32_t)bpm, (int)(blk % (uint32_t)bpm), &c);
        first[idx] = blk_first; count[idx] = 0;
    }
    if (iters) *iters = it;
    return damage;
}

}  // namespace jmamd
