// jmcodec_amd/csrc/mpeg2_vlc.h -- MPEG-2 (codec_type 4), option mpeg2_device_vlc: the slice / macroblock / block VLC decode of ONE slice as a
// __host__ __device__ routine.  k_mpeg2_vlc (mpeg2_kernels.hip) runs it with one lane per slice; tests/native/mpeg2_vlc_check.cpp and
// tools/mpeg2_vlc_asan.cpp walk the same code on the CPU.  No HIP header: g++ builds it.  It restates SliceDec::slice, macroblock, motion_vectors,
// mv_component, block, skipped and clamp_vectors of mpeg2_syntax.cpp over a 64-bit bit window.
//
// What the device is given (built by mpeg2_slice_scan, mpeg2_syntax.cpp; layout of the uploaded blob: INTEGRATION.md "MPEG-2"):
//   picture   Mpeg2VlcPic: the fields of the picture header and coding extension that the VLC needs, 64 bytes;
//   slices    Mpeg2Slice[n]: where the slice's bytes start, how many there are, its macroblock row, the span [lo, hi) of macroblock addresses it
//             owns, where its entries go and how many fit.  The prescan reads the slice header and the first macroblock_address_increment only to
//             learn the slice's first macroblock address s; THE LANE REPEATS THE HEADER (quantiser_scale_code, the extra-information bits, the
//             first increment) from the slice's first bit -- no bit position travels.  lo_0 = 0, lo_i = s_i; hi_i = s_{i+1}, the last hi = mb_w mb_h:
//             the spans tile the picture, every record has exactly one writer;
//   bytes     per slice the bytes behind its start code, copied to an offset that is a multiple of 4, padded with zeros to a multiple of 4 and
//             followed by kMpeg2SliceGuard zero bytes: the reader takes whole aligned dwords, and bits behind the slice read as zeros, which is what
//             the host's Bits::peek supplies;
//   tables    Mpeg2VlcTables, built once per process from mpeg2_table() (mpeg2_vlc_tables, mpeg2_syntax.cpp), uploaded once per engine.
//
// Tables: every table but the DCT coefficients' is one level, indexed by the next maxlen bits -- B-1 11 bits (2048 entries), B-2 / B-3 / B-4 6 bits
// (3 x 64), B-9 9 bits (512), B-10 10 bits (1024), B-12 9 bits (512), B-13 10 bits (1024); an entry is length | (a + 1) << 5, 0 = no such code.
// B-14 and B-15 (codes of up to 16 bits) have two levels: every code longer than 8 bits begins with six zero bits (the builder checks this), so
// level 1 is indexed by the next 8 bits (256 entries) and, when the first six are zero, level 2 by bits 6..15 (1024 entries); an entry is
// (length - 1) | run << 4 | level << 10 with run 62 = escape, 63 = end of block; 0 = no such code.  With the two scans (128 bytes) and the two
// quantiser_scale tables (64 bytes): 2 x (2048 + 192 + 512 + 1024 + 512 + 1024 + 2 x 1280) + 192 = 15,936 bytes.
//
// The guard.  The window holds n valid bits and is topped up with one dword whenever n <= 32, before every read (the dword behind it is loaded at the
// same moment, one ahead); a read takes at most 24 bits.  The
// host's decoder looks at `over` (a bit beyond 8 L was consumed) at the head of the macroblock loop, behind every coefficient and at the end of every
// macroblock, and the routine stops at the same places.  From a check that passed (position <= 8 L) to the next one the longest chain of reads is:
// an address increment that straddles the end (11 bits), macroblock_type 6, frame_motion_type 2, dct_type 1, quantiser_scale_code 5, four vectors of
// 1 + 2 (10 + 1 + 8) bits = 156, coded_block_pattern 9 -- 190 bits -- and then either six intra blocks of a DC symbol (10 + 11) and an end of block
// (4) with no coefficient between them, 150 bits, or one coefficient of at most 24: at most 340 bits.  The window is at most 64 bits ahead of the
// position and the load one dword ahead of the window, so no bit beyond 8 L + 436 is fetched: 55 bytes; pad4(L) + 56 covers it.  The reader checks its dword index against that size all the same
// and supplies zeros beyond it, so a slice never sees another slice's bytes.
//
// Entry capacity of a span of M macroblocks whose slice has L bytes: min(384 M, 4 L + 6 M).
//   A macroblock has 6 blocks of at most 64 entries.  Every entry the routine KEEPS costs at least 2 bits of the slice: the cheapest are the first
//   coefficient of a non-intra block, `1s`, and a chroma DC of size 0 behind a non-zero predictor, `00`; a macroblock that consumed a bit beyond 8 L
//   is dropped with its entries, so kept entries number at most 4 L.  A concealed macroblock of an I picture writes 6 entries and reads no bits, and
//   there are at most M of them.  Entries of the macroblock being decoded are written before it is known to be kept: those whose symbols end inside
//   the slice are among the 4 L, and at most 6 DC entries can follow beyond the end (every AC entry is written behind a check of `over`) -- 6 M
//   covers them, since the macroblock being decoded is not concealed yet.  The routine checks every write against the capacity all the same and
//   treats an overflow as damage (kM2DmgCapacity).
//
// Loops.  Every macroblock iteration consumes an address increment (at least 1 bit) and moves the address forward, so there are at most M of them
// per lane that stay inside the span (one more may end the lane); an escape consumes 11 bits and adds 33 to the increment, and the loop ends once the
// increment exceeds mb_w mb_h; the coefficient loop moves the position n forward by at least one per iteration and ends at n > 63, so it runs at
// most 65 times per block and each iteration but the last consumes at least 2 bits; the extra-information loop consumes 9 bits per iteration and
// ends on `over`; the skipped loop and the concealment loops run at most M times each, together at most M (an address is written once).  In all:
// iterations <= 8 L + 2 M + 512 -- the for-loops carry their limits, and the CPU walk asserts the count.
//
// Damage: the kinds below, in the host path's wording (mpeg2_vlc_damage_text).  The macroblock that met it and the rest of the SLICE are dropped; every
// address of the span that no decoded or skipped macroblock covered is concealed as the tail of mpeg2_decode_picture does -- zero-vector forward
// records with qscale 2 in P and B pictures, intra records with six DC entries of 128 << intra_dc_precision in I pictures -- and the status says
// "holes".  A macroblock at or beyond `hi` ends the lane silently: on the host path the next slice overwrites it.  frame_motion_type 3 (dual prime):
// when Mpeg2VlcPic::dual_prime is set (option mpeg2_field_pictures) the lane decodes it as the host does -- one vector in field format, a dmvector
// (one or two bits, read without a table) behind each component, the derived vectors from mpeg2_dual_vector, the host's clamp -- and writes the host's
// record (M2_DUAL; in a B picture it is damage); 44 bits at most, fewer than the four vectors the guard's chain allows for.  Otherwise it sets its own
// status bit and ends the lane like damage; the handle fails when the engine reads it.
#pragma once
#include <stdint.h>
#include "mpeg2_jobs.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define M2V_HD __host__ __device__ __forceinline__
#else
#define M2V_HD inline
#endif
// The slice bytes, the records and the entries are device allocations.  In the device pass the routine addresses them through global-memory pointers:
// through generic ones every load and store would be a flat instruction, which shares the LDS counter that each table read waits on.
#if defined(__HIP_DEVICE_COMPILE__)
#define M2V_GLOBAL __attribute__((address_space(1)))
#else
#define M2V_GLOBAL
#endif

namespace jmamd {

constexpr int kMpeg2SliceGuard = 56;       // zero bytes behind every slice's padded bytes

struct Mpeg2VlcTables {
    uint16_t mba[2048];                    // B-1: a = increment, 34 = escape
    uint16_t mbtype[3][64];                // B-2, B-3, B-4 by picture_coding_type - 1
    uint16_t cbp[512], motion[1024], dc_luma[512], dc_chroma[1024];
    uint16_t dct[2][1280];                 // B-14, B-15: [0..255] level 1, [256..1279] level 2
    uint8_t scan[2][64];                   // kMpeg2Scan
    uint8_t qscale[2][32];                 // mpeg2_quantiser_scale(q_scale_type, code)
};
static_assert(sizeof(Mpeg2VlcTables) == 15936, "the device form of the Annex B tables is 15,936 bytes");

struct Mpeg2VlcPic {                       // 64 bytes
    int32_t type;                          // picture_coding_type: 1 I, 2 P, 3 B
    int32_t f_code[2][2];
    int32_t intra_dc_precision, frame_pred_frame_dct, concealment_mv, q_scale_type, intra_vlc_format, alternate_scan;
    int32_t mb_w, mb_h;
    int32_t dual_prime;                    // option mpeg2_field_pictures: the lane decodes frame_motion_type 3 (0: it reports kM2StDualPrime, the handle fails)
    int32_t top_field_first;               // ... which needs it: which derived vector of a dual-prime macroblock is scaled by 1 and which by 3
    int32_t pad[1];
};
static_assert(sizeof(Mpeg2VlcPic) == 64, "Mpeg2VlcPic is 64 bytes");

struct Mpeg2Slice {                        // 32 bytes
    uint32_t byte_off;                     // of its bytes, from the start of the picture's slice bytes; a multiple of 4
    uint32_t n_bytes;                      // L: the bytes behind the start code
    uint32_t row;                          // slice_vertical_position - 1
    uint32_t lo, hi;                       // the macroblock addresses it owns
    uint32_t first_entry, entry_cap;       // its entries go to entries[first_entry .. first_entry + entry_cap)
    uint32_t pad;
};
static_assert(sizeof(Mpeg2Slice) == 32, "Mpeg2Slice is 32 bytes");

M2V_HD uint32_t mpeg2_vlc_capacity(uint32_t n_bytes, uint32_t n_mbs) {
    const uint64_t a = 384ull * n_mbs, b = 4ull * n_bytes + 6ull * n_mbs;
    return (uint32_t)(a < b ? a : b);
}
// bytes a slice of L bytes takes in the uploaded byte array
M2V_HD uint32_t mpeg2_vlc_padded(uint32_t n_bytes) { return ((n_bytes + 3u) & ~3u) + (uint32_t)kMpeg2SliceGuard; }
// the stated bound of the routine's loop iterations
M2V_HD long long mpeg2_vlc_iteration_bound(uint32_t n_bytes, uint32_t n_mbs) { return 8ll * n_bytes + 2ll * n_mbs + 512; }

// kinds of damage (the value in bits 0..4 of the routine's result; the picture's status word collects 1 << kind)
enum : int {
    kM2DmgNone = 0, kM2DmgFcode, kM2DmgMotionCode, kM2DmgDcSize, kM2DmgDcRange, kM2DmgDctCode, kM2DmgEmptyBlock, kM2DmgEscapeLevel, kM2DmgBlockLength,
    kM2DmgMbType, kM2DmgMotionType, kM2DmgQuantCode, kM2DmgMarker, kM2DmgNoPrediction, kM2DmgCbp, kM2DmgSliceEnd, kM2DmgIncrement, kM2DmgAddress,
    kM2DmgSkippedInI, kM2DmgCapacity, kM2DmgDualPrime, kM2DmgDualPrimeInB, kM2DmgKinds
};
// the routine's result: kind of damage | holes concealed | dual prime met | clamped macroblocks << 8
constexpr uint32_t kM2StKindMask = 31, kM2StHoles = 32, kM2StDualPrime = 64;
constexpr int kM2StClampedShift = 8;

inline const char *mpeg2_vlc_damage_text(int kind) {
    static const char *const t[kM2DmgKinds] = {"", "an f_code outside 1..9 is used", "invalid motion_code", "invalid dct_dc_size", "an intra DC coefficient out of range",
        "invalid DCT coefficient code", "an empty coded block", "a forbidden escape level", "a block with more than 64 coefficients", "invalid macroblock_type",
        "reserved frame_motion_type", "quantiser_scale_code 0", "the marker bit behind concealment vectors is 0", "a macroblock without prediction in a B picture",
        "invalid coded_block_pattern", "a slice ends inside a macroblock", "invalid macroblock_address_increment", "a macroblock address beyond the picture",
        "a skipped macroblock in an I picture", "more entries than the slice's bytes can code", "dual-prime prediction is not supported",
        "dual-prime prediction in a B picture"};
    return kind > 0 && kind < kM2DmgKinds ? t[kind] : "";
}

// 7.6.3.6: one vector of the opposite parity of a dual-prime macroblock from the transmitted vector (vx, vy) and dmvector: m = 1 or 3, e = -1 when
// the lines predicted belong to a top field, +1 to a bottom field.  The host's slice decode and the lane both call this: one copy of the arithmetic
M2V_HD void mpeg2_dual_vector(int vx, int vy, int dmv0, int dmv1, int m, int e, int *x, int *y) {
    *x = ((vx * m + (vx > 0 ? 1 : 0)) >> 1) + dmv0;
    *y = ((vy * m + (vy > 0 ? 1 : 0)) >> 1) + e + dmv1;
}

namespace m2v {

struct alignas(16) Quad { uint32_t x, y, z, w; };

// MSB-first reader over the slice's padded dwords: n valid bits at the top of acc, wi dwords taken into the window so far, pos bits consumed.
// nxt holds dword wi, loaded when dword wi - 1 went into the window: a refill uses a value that has been on its way for 32 bits' worth of symbols
// and starts the next load, so the lane does not wait a memory round trip at the refill itself (64 lanes refill at unrelated moments, and the wave
// would otherwise wait one at nearly every read).  Every load's index is checked against the padded size.
struct Bits {
    const M2V_GLOBAL uint32_t *w; uint32_t n_words, wi; uint64_t acc; int n; long long pos, end_bit; bool over; uint32_t nxt;
    M2V_HD void start() { nxt = n_words ? w[0] : 0u; }
    M2V_HD void fill() { if (n <= 32) { acc |= (uint64_t)__builtin_bswap32(nxt) << (32 - n); n += 32; wi++; nxt = wi < n_words ? w[wi] : 0u; } }
    M2V_HD uint32_t peek(int k) { fill(); return (uint32_t)(acc >> (64 - k)); }                        // 1 <= k <= 24
    M2V_HD void skip(int k) { fill(); acc <<= k; n -= k; pos += k; if (pos > end_bit) over = true; }   // 0 <= k <= 24
    M2V_HD uint32_t get(int k) { if (k == 0) return 0; const uint32_t v = peek(k); skip(k); return v; }
    // the same without the top-up, for a run of reads that one fill() covers (at least 33 bits are in the window behind it)
    M2V_HD uint32_t peek_raw(int k) const { return (uint32_t)(acc >> (64 - k)); }
    M2V_HD void skip_raw(int k) { acc <<= k; n -= k; pos += k; if (pos > end_bit) over = true; }
    M2V_HD uint32_t get_raw(int k) { const uint32_t v = peek_raw(k); skip_raw(k); return v; }
    M2V_HD long long left() const { return pos < end_bit ? end_bit - pos : 0; }
};

// one symbol of a one-level table: its a, or -1 for an invalid code
M2V_HD int vlc(Bits &b, const uint16_t *look, int maxlen) {
    const uint32_t e = look[b.peek(maxlen)];
    if (!e) return -1;
    b.skip((int)(e & 31));
    return (int)(e >> 5) - 1;
}

struct State {
    int pmv[2][2][2];                      // [r][s][t]: indexed by constants only (the loops over r are unrolled, s is a template argument)
    int dc0, dc1, dc2;                     // dc_pred of Y, Cb, Cr
    int qscale; uint32_t prev_dir;
    uint32_t clamped;
};
M2V_HD void reset_pmv(State &st) {
    st.pmv[0][0][0] = st.pmv[0][0][1] = st.pmv[0][1][0] = st.pmv[0][1][1] = 0;
    st.pmv[1][0][0] = st.pmv[1][0][1] = st.pmv[1][1][0] = st.pmv[1][1][1] = 0;
}

// 7.6.3.1: one component from its predictor; 0 or the kind of damage
M2V_HD int mv_component(Bits &b, const Mpeg2VlcTables *t, int f_code, int pred, int *out) {
    if (f_code < 1 || f_code > 9) return kM2DmgFcode;
    const int m = vlc(b, t->motion, 10);
    if (m < 0) return kM2DmgMotionCode;
    int delta = 0;
    if (m) {
        const bool neg = b.get(1) != 0;
        const int r_size = f_code - 1;
        delta = ((m - 1) << r_size) + (int)b.get(r_size) + 1;
        if (neg) delta = -delta;
    }
    const int f = 1 << (f_code - 1), lo = -16 * f, hi = 16 * f - 1;
    int v = pred + delta;
    if (v < lo) v += 32 * f; else if (v > hi) v -= 32 * f;
    *out = v;
    return 0;
}
M2V_HD uint32_t pack_mv(int x, int y) { return (uint32_t)(uint16_t)(int16_t)x | (uint32_t)(uint16_t)(int16_t)y << 16; }

// motion_vectors(S) of a frame picture: the vectors land in mv0 (r = 0) and mv1 (r = 1), the field selects in *flags
template <int S> M2V_HD int motion_vectors(Bits &b, const Mpeg2VlcTables *t, const Mpeg2VlcPic &pic, State &st, bool field, uint32_t *flags, uint32_t *mv0, uint32_t *mv1) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int r = 0; r < 2; r++) {
        if (r == 1 && !field) break;
        if (field) *flags |= b.get(1) << (M2_SEL_SHIFT + 2 * S + r);
        int x = 0, y = 0;
        if (const int d = mv_component(b, t, pic.f_code[S][0], st.pmv[r][S][0], &x)) return d;
        if (const int d = mv_component(b, t, pic.f_code[S][1], field ? st.pmv[r][S][1] >> 1 : st.pmv[r][S][1], &y)) return d;
        st.pmv[r][S][0] = x; st.pmv[r][S][1] = field ? y * 2 : y;
        *(r ? mv1 : mv0) = pack_mv(x, y);
    }
    if (!field) { st.pmv[1][S][0] = st.pmv[0][S][0]; st.pmv[1][S][1] = st.pmv[0][S][1]; }
    return 0;
}

// B-11 dmvector: 0 -> 0, 10 -> 1, 11 -> -1 (two bits at most: read from the window, no table)
M2V_HD int dmvector(Bits &b) { if (!b.get(1)) return 0; return b.get(1) ? -1 : 1; }

// motion_vectors(0) of a dual-prime macroblock of a P frame picture (the host's kDual): one vector in field format -- the vertical predictor halved,
// stored back doubled -- a dmvector behind each component, PMV[1] = PMV[0]; mv0 = the vector, mv2 / mv3 = the derived vectors of the top / bottom lines
M2V_HD int dual_vectors(Bits &b, const Mpeg2VlcTables *t, const Mpeg2VlcPic &pic, State &st, uint32_t *mv0, uint32_t *mv2, uint32_t *mv3) {
    int x = 0, y = 0, dx, dy;
    if (const int d = mv_component(b, t, pic.f_code[0][0], st.pmv[0][0][0], &x)) return d;
    const int dmv0 = dmvector(b);
    if (const int d = mv_component(b, t, pic.f_code[0][1], st.pmv[0][0][1] >> 1, &y)) return d;
    const int dmv1 = dmvector(b);
    st.pmv[0][0][0] = st.pmv[1][0][0] = x; st.pmv[0][0][1] = st.pmv[1][0][1] = y * 2;
    *mv0 = pack_mv(x, y);
    mpeg2_dual_vector(x, y, dmv0, dmv1, pic.top_field_first ? 1 : 3, -1, &dx, &dy); *mv2 = pack_mv(dx, dy);
    mpeg2_dual_vector(x, y, dmv0, dmv1, pic.top_field_first ? 3 : 1, 1, &dx, &dy); *mv3 = pack_mv(dx, dy);
    return 0;
}

// clamp_vectors on one packed vector
M2V_HD uint32_t clamp_one(uint32_t v, int x_lo, int x_hi, int y_lo, int y_hi, bool *cl) {
    const int vx = (int16_t)(v & 0xffff), vy = (int16_t)(v >> 16);
    const int x = vx < x_lo ? x_lo : (vx > x_hi ? x_hi : vx), y = vy < y_lo ? y_lo : (vy > y_hi ? y_hi : vy);
    if (x != vx || y != vy) *cl = true;
    return pack_mv(x, y);
}

// the record as the eight dwords of Mpeg2Mb (little endian), stored as two 16-byte stores
struct Rec { uint32_t flags, qscale, cbp, mv[4], first; uint64_t counts; };
M2V_HD void put(M2V_GLOBAL Mpeg2Mb *mbs, const Mpeg2VlcPic &pic, State &st, uint32_t addr, Rec r) {
    if (!(r.flags & M2_INTRA)) {
        const int mx = (int)(addr % (uint32_t)pic.mb_w), my = (int)(addr / (uint32_t)pic.mb_w), W = pic.mb_w * 16, H = pic.mb_h * 16;
        const bool dual = (r.flags & M2_DUAL) != 0, field = (r.flags & M2_FIELD_MV) != 0 || dual;      // (dual prime: 8 lines of a field, as field vectors)
        const int x_lo = -2 * mx * 16, x_hi = 2 * (W - 16 - mx * 16);
        const int y_lo = field ? -2 * my * 8 : -2 * my * 16, y_hi = field ? 2 * (H / 2 - 8 - my * 8) : 2 * (H - 16 - my * 16);
        bool cl = false;
        if (dual) { r.mv[0] = clamp_one(r.mv[0], x_lo, x_hi, y_lo, y_hi, &cl); r.mv[2] = clamp_one(r.mv[2], x_lo, x_hi, y_lo, y_hi, &cl); r.mv[3] = clamp_one(r.mv[3], x_lo, x_hi, y_lo, y_hi, &cl); }
        else if (r.flags & M2_FWD) { r.mv[0] = clamp_one(r.mv[0], x_lo, x_hi, y_lo, y_hi, &cl); if (field) r.mv[1] = clamp_one(r.mv[1], x_lo, x_hi, y_lo, y_hi, &cl); }
        if (!dual && (r.flags & M2_BWD)) { r.mv[2] = clamp_one(r.mv[2], x_lo, x_hi, y_lo, y_hi, &cl); if (field) r.mv[3] = clamp_one(r.mv[3], x_lo, x_hi, y_lo, y_hi, &cl); }
        if (cl) { r.flags |= M2_CLAMPED; st.clamped++; }
    }
    M2V_GLOBAL Quad *q = (M2V_GLOBAL Quad *)(mbs + addr);
    const Quad a = {r.flags | r.qscale << 16 | r.cbp << 24, r.mv[0], r.mv[1], r.mv[2]};
    const Quad c = {r.mv[3], r.first, (uint32_t)r.counts, (uint32_t)(r.counts >> 32)};
    q[0] = a; q[1] = c;
}

}  // namespace m2v

// Decodes slice sl of picture pic.  t: the tables; bytes: the picture's slice bytes (4-byte aligned); mbs: the picture's records (16-byte aligned);
// entries: the picture's entry list.  Writes the record of every address in [sl.lo, sl.hi) and their entries; returns the status (kM2St*).
// *iters (may be null) receives the number of loop iterations, *n_dual (may be null) the number of dual-prime records written.
M2V_HD uint32_t mpeg2_vlc_slice(const Mpeg2VlcPic &pic, const Mpeg2VlcTables *t, const Mpeg2Slice &sl, const uint32_t *bytes_, Mpeg2Mb *mbs_,
                                uint32_t *entries_, long long *iters, uint32_t *n_dual = nullptr) {
    using namespace m2v;
    const M2V_GLOBAL uint32_t *bytes = (const M2V_GLOBAL uint32_t *)bytes_;
    M2V_GLOBAL Mpeg2Mb *mbs = (M2V_GLOBAL Mpeg2Mb *)mbs_;
    M2V_GLOBAL uint32_t *entries = (M2V_GLOBAL uint32_t *)entries_;
    const uint32_t total = (uint32_t)pic.mb_w * (uint32_t)pic.mb_h, M = sl.hi - sl.lo;
    const uint32_t e_end = sl.first_entry + sl.entry_cap;
    const bool is_i = pic.type == 1;
    const int dc_reset = 1 << (pic.intra_dc_precision + 7), dc_limit = 1 << (8 + pic.intra_dc_precision);
    Bits b = {bytes + (sl.byte_off >> 2), mpeg2_vlc_padded(sl.n_bytes) >> 2, 0, 0, 0, 0, 8ll * sl.n_bytes, false, 0};
    b.start();
    State st = {};
    uint32_t e = sl.first_entry, next = sl.lo;          // next: the lowest address of the span that has no record yet
    int damage = 0; bool holes = false;
    long long it = 0; uint32_t duals = 0;

    // a concealed macroblock: what the tail of mpeg2_decode_picture writes
    auto conceal = [&](uint32_t from, uint32_t to) {
        for (uint32_t a = from, j = 0; a < to && j < M; a++, j++, it++) {
            Rec r = {}; r.first = e; r.qscale = 2;
            if (is_i) {
                r.flags = M2_INTRA; r.cbp = 63;
                if (e + 6 <= e_end) { for (int k = 0; k < 6; k++) entries[e++] = (uint32_t)(128 << pic.intra_dc_precision) << 16; r.counts = 0x010101010101ull; }
                else damage = damage ? damage : kM2DmgCapacity;       // (not reachable within the stated capacity: the record is an empty intra block)
            } else r.flags = M2_FWD;
            m2v::put(mbs, pic, st, a, r);
            holes = true;
        }
    };

    // ---- the slice header, as the prescan read it ----
    { const int c = (int)b.get(5); if (c == 0) damage = kM2DmgQuantCode; st.qscale = t->qscale[pic.q_scale_type & 1][c & 31]; }
    if (!damage && b.get(1)) { b.skip(8); for (long long j = 0; j <= b.end_bit / 9 + 1 && b.get(1) && !b.over; j++, it++) b.skip(8); }
    st.dc0 = st.dc1 = st.dc2 = dc_reset; st.prev_dir = M2_FWD;
    uint32_t prev = sl.row * (uint32_t)pic.mb_w - 1u; bool first = true;          // (row 0: prev = -1 in 32-bit arithmetic, as the host's int)
    for (uint32_t mb_it = 0; !damage && mb_it <= M && !b.over && b.left() > 0 && b.peek(23) != 0; mb_it++, it++) {
        // macroblock_address_increment with its escapes
        uint32_t inc = 0;
        for (;;) {
            const int m = vlc(b, t->mba, 11);
            if (m < 0) { damage = kM2DmgIncrement; break; }
            it++;
            if (m == 34) { inc += 33; if (inc > total) { damage = kM2DmgAddress; break; } continue; }
            inc += (uint32_t)m; break;
        }
        if (damage) break;
        const uint32_t addr = prev + inc;
        if (addr >= total) { damage = kM2DmgAddress; break; }
        if (!first && inc > 1 && is_i) { damage = kM2DmgSkippedInI; break; }
        if (first && addr > next) { const uint32_t to = addr < sl.hi ? addr : sl.hi; conceal(next, to); next = to; if (damage) break; }      // [lo_0, s_0): only the first lane has such a gap
        if (!first && inc > 1) {
            // skipped macroblocks: P a zero vector, the predictors and the DC reset; B the direction(s) of the macroblock before, frame prediction
            const uint32_t to = addr < sl.hi ? addr : sl.hi;
            for (uint32_t a = prev + 1, j = 0; a < to && j < M; a++, j++, it++) {
                Rec r = {}; r.first = e; r.qscale = (uint32_t)st.qscale;
                st.dc0 = st.dc1 = st.dc2 = dc_reset;
                if (pic.type == 2) { reset_pmv(st); r.flags = M2_FWD; }
                else { r.flags = st.prev_dir; r.mv[0] = pack_mv(st.pmv[0][0][0], st.pmv[0][0][1]); r.mv[2] = pack_mv(st.pmv[0][1][0], st.pmv[0][1][1]); }
                m2v::put(mbs, pic, st, a, r);
            }
            if (to > next) next = to;
        }
        if (addr >= sl.hi) break;                                   // the next slice's: not damage
        // ---- macroblock() ----
        const uint32_t e0 = e;
        int dmg = 0;
        Rec rec = {};
        do {
            const int ty = vlc(b, t->mbtype[is_i ? 0 : (pic.type == 2 ? 1 : 2)], 6);
            if (ty < 0) { dmg = kM2DmgMbType; break; }
            const bool quant = ty & 1, mf = (ty & 2) != 0, mbk = (ty & 4) != 0, pattern = (ty & 8) != 0, intra = (ty & 16) != 0;
            bool field_mv = false, field_dct = false, dual = false;
            if ((mf || mbk) && !pic.frame_pred_frame_dct) {
                const int fmt = (int)b.get(2);
                if (fmt == 3) {
                    if (!pic.dual_prime) { dmg = kM2DmgDualPrime; break; }
                    if (pic.type != 2 || !mf) { dmg = kM2DmgDualPrimeInB; break; }
                    dual = true;
                }
                if (fmt == 0) { dmg = kM2DmgMotionType; break; }
                field_mv = fmt == 1;
            }
            if (!pic.frame_pred_frame_dct && (intra || pattern)) field_dct = b.get(1) != 0;
            if (quant) { const int c = (int)b.get(5); if (c == 0) { dmg = kM2DmgQuantCode; break; } st.qscale = t->qscale[pic.q_scale_type & 1][c]; }
            rec.first = e; rec.qscale = (uint32_t)st.qscale;
            if (field_dct) rec.flags |= M2_FIELD_DCT;
            if (intra) {
                rec.flags |= M2_INTRA;
                if (pic.concealment_mv) {
                    uint32_t f = 0, v0 = 0, v1 = 0;
                    if ((dmg = motion_vectors<0>(b, t, pic, st, false, &f, &v0, &v1)) != 0) break;
                    if (!b.get(1)) { dmg = kM2DmgMarker; break; }
                } else reset_pmv(st);
            } else {
                st.dc0 = st.dc1 = st.dc2 = dc_reset;
                if (dual) { rec.flags |= M2_FWD | M2_DUAL; if ((dmg = dual_vectors(b, t, pic, st, &rec.mv[0], &rec.mv[2], &rec.mv[3])) != 0) break; }
                else if (mf) { rec.flags |= M2_FWD; if ((dmg = motion_vectors<0>(b, t, pic, st, field_mv, &rec.flags, &rec.mv[0], &rec.mv[1])) != 0) break; }
                if (mbk) { rec.flags |= M2_BWD; if ((dmg = motion_vectors<1>(b, t, pic, st, field_mv, &rec.flags, &rec.mv[2], &rec.mv[3])) != 0) break; }
                if (field_mv) rec.flags |= M2_FIELD_MV;
                if (!mf && !mbk) {
                    if (pic.type != 2) { dmg = kM2DmgNoPrediction; break; }
                    rec.flags |= M2_FWD; reset_pmv(st);
                }
                st.prev_dir = rec.flags & (M2_FWD | M2_BWD);
            }
            int cbp = intra ? 63 : 0;
            if (pattern) { const int c = vlc(b, t->cbp, 9); if (c <= 0) { dmg = kM2DmgCbp; break; } cbp = c; }
            rec.cbp = (uint32_t)cbp;
            const uint16_t *dct = t->dct[intra && pic.intra_vlc_format ? 1 : 0];
            const uint8_t *scan = t->scan[pic.alternate_scan ? 1 : 0];
            for (int k = 0; k < 6 && !dmg; k++) {
                if (!(cbp & (32 >> k))) continue;
                // ---- block(k) ----
                const uint32_t eb = e;
                int n = 0;
                if (intra) {
                    const int size = k < 4 ? vlc(b, t->dc_luma, 9) : vlc(b, t->dc_chroma, 10);
                    if (size < 0) { dmg = kM2DmgDcSize; break; }
                    int diff = 0;
                    if (size) { const int v = (int)b.get(size), half = 1 << (size - 1); diff = v >= half ? v : v + 1 - 2 * half; }
                    const int pred = (k < 4 ? st.dc0 : (k == 4 ? st.dc1 : st.dc2)) + diff;
                    if (k < 4) st.dc0 = pred; else if (k == 4) st.dc1 = pred; else st.dc2 = pred;
                    if (pred < 0 || pred >= dc_limit) { dmg = kM2DmgDcRange; break; }
                    if (pred) { if (e >= e_end) { dmg = kM2DmgCapacity; break; } entries[e++] = (uint32_t)pred << 16; }
                    n = 1;
                }
                bool done = false;
                for (int j = 0; j < 65 && !done; j++, it++) {
                    int run, level;
                    b.fill();                 // one top-up per coefficient: it takes at most 24 bits (escape: 6 + 6 + 12) of the 33 or more now in the window
                    if (!intra && n == 0 && b.peek_raw(1)) { b.skip_raw(1); run = 0; level = b.get_raw(1) ? -1 : 1; }
                    else {
                        const uint32_t v16 = b.peek_raw(16);
                        const uint32_t c = (v16 >> 10) ? dct[v16 >> 8] : dct[256 + (v16 & 1023)];
                        if (!c) { dmg = kM2DmgDctCode; break; }
                        b.skip_raw((int)(c & 15) + 1);
                        const int crun = (int)(c >> 4 & 63), clevel = (int)(c >> 10);
                        if (crun == 63) { if (!intra && n == 0) dmg = kM2DmgEmptyBlock; done = true; break; }
                        if (crun == 62) {
                            run = (int)b.get_raw(6); level = (int)b.get_raw(12); if (level >= 2048) level -= 4096;
                            if (level == 0 || level == -2048) { dmg = kM2DmgEscapeLevel; break; }
                        } else { run = crun; level = b.get_raw(1) ? -clevel : clevel; }
                    }
                    n += run;
                    if (n > 63 || b.over) { dmg = kM2DmgBlockLength; break; }
                    if (e >= e_end) { dmg = kM2DmgCapacity; break; }
                    entries[e++] = (uint32_t)scan[n] | (uint32_t)(uint16_t)(int16_t)level << 16;
                    n++;
                }
                if (dmg) break;
                if (!done) { dmg = kM2DmgBlockLength; break; }         // (not reachable: n moves forward in every iteration)
                rec.counts |= (uint64_t)((e - eb) & 255u) << (8 * k);
            }
            if (dmg) break;
            if (b.over) { dmg = kM2DmgSliceEnd; break; }
        } while (false);
        if (dmg) { e = e0; damage = dmg; break; }
        m2v::put(mbs, pic, st, addr, rec);
        if (rec.flags & M2_DUAL) duals++;
        next = addr + 1; prev = addr; first = false;
    }
    // every address of the span that has no record yet
    if (next < sl.hi) conceal(next, sl.hi);
    if (iters) *iters = it;
    if (n_dual) *n_dual = duals;
    return (uint32_t)damage | (holes ? kM2StHoles : 0u) | (damage == kM2DmgDualPrime ? kM2StDualPrime : 0u) | st.clamped << kM2StClampedShift;
}

}  // namespace jmamd
