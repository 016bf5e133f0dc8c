// jmcodec_amd/csrc/vp8_jobs.h -- what the host hands k_vp8_inter, k_vp8_recon and k_vp8_filter for one VP8 frame (codec_type 5; INTEGRATION.md "VP8").
//
// The host resolves the whole syntax (bool decoder, modes, tokens: vp8_syntax.cpp): one fixed 32-byte record per macroblock in raster order and a
// SPARSE entry list in the style of jpeg_jobs.h / mpeg2_jobs.h -- one 32-bit entry per non-zero level:
//     bits 0..3  raster position inside the 4x4 block (the zig-zag already applied)
//     bits 4..8  block of the macroblock: 0..15 luma in raster order, 16..19 U, 20..23 V, 24 the Y2 block
//     bits 16..31 the quantised level (int16; |level| <= 2114 by the token syntax)
// The entries of a macroblock are contiguous from `first`.  The device dequantises with the picture's per-segment factors (the product truncated to
// int16, as the RFC's and libwebp's coefficient arrays are), runs the inverse WHT and the IDCTs, predicts and stores.  Every field the device indexes
// with is validated by the host (vp8_validate_jobs) and clamped again where it is used.
#pragma once
#include <stdint.h>

struct ihipStream_t;

namespace jmamd {

enum : uint8_t {
    VP8_MB_INNER = 1,      // the loop filter also filters the macroblock's inner edges: B_PRED, SPLITMV, or some block has coefficients (RFC 6386 15.1... 15.3)
    VP8_MB_INTER = 2       // option vp8_inter: predicted from a reference frame by k_vp8_inter; k_vp8_recon leaves it alone.  The bmodes bytes then hold
                           // a Vp8InterInfo, and ymode says only whether there is a Y2 block: VP8_B_PRED for SPLITMV (none), VP8_DC_PRED otherwise
};
// the vector modes, numbered as the mv_ref tree yields them + 1 (Vp8Mb::mvmode; 0 = intra)
enum : uint8_t { VP8_MV_ZERO = 1, VP8_MV_NEAREST, VP8_MV_NEAR, VP8_MV_NEW, VP8_MV_SPLIT };
// 16x16 luma / chroma modes and the sub-block modes, numbered as in the RFC
enum : uint8_t { VP8_DC_PRED = 0, VP8_V_PRED, VP8_H_PRED, VP8_TM_PRED, VP8_B_PRED };
enum : uint8_t { VP8_B_DC = 0, VP8_B_TM, VP8_B_VE, VP8_B_HE, VP8_B_LD, VP8_B_RD, VP8_B_VR, VP8_B_VL, VP8_B_HD, VP8_B_HU };

constexpr int kVp8MaxMbEntries = 25 * 16;

struct Vp8Mb {             // 32 bytes
    uint32_t first;        // index of the macroblock's first entry
    uint16_t count;        // its entries (0 .. 400)
    uint8_t ymode;         // VP8_DC_PRED .. VP8_B_PRED
    uint8_t uvmode;        // VP8_DC_PRED .. VP8_TM_PRED
    uint8_t segment;       // 0..3: selects Vp8PicParams::dq
    uint8_t level;         // loop filter level, resolved (segment, delta_enable and the intra / B_PRED deltas applied, clamped): 0..63, 0 = not filtered
    uint8_t flags;         // VP8_MB_*
    uint8_t mvmode;        // 0 intra, VP8_MV_* (the device reads VP8_MV_SPLIT alone; a key frame's records hold 0)
    uint32_t nz;           // bit b: block b (numbered as in the entries) has at least one entry
    uint8_t bmodes[16];    // B_PRED: the sub-block modes in raster order (else the implied modes; the device does not read them then)
};
static_assert(sizeof(Vp8Mb) == 32, "Vp8Mb is 32 bytes");

// Vectors are in eighth samples of the plane they address: (v >> 3) whole samples and (v & 7) the fraction.  Luma fractions are even.  They are
// arbitrary 16-bit values (sums of what a stream codes): the device clamps the COORDINATES they lead to, never the vectors.
struct Vp8InterInfo {      // the 16 bmodes bytes of an inter macroblock
    uint8_t ref;           // 1 last, 2 golden, 3 altref
    uint8_t split;         // SPLITMV: 1 + the partitioning (0 16x8, 1 8x16, 2 8x8, 3 4x4); else 0
    uint8_t pad[2];
    int16_t mvx, mvy;      // the macroblock's luma vector (SPLITMV: that of block 15)
    int16_t cmvx, cmvy;    // the chroma vector the host derived (RFC 6386 section 5, the decoder's build of the chroma vectors; version 3: fraction cleared)
    uint32_t split_idx;    // SPLITMV: index into Vp8PicParams::split
};
static_assert(sizeof(Vp8InterInfo) == 16, "Vp8InterInfo overlays bmodes");
struct Vp8SplitMv {        // 80 bytes: per luma block in raster order, then per chroma block (U and V share them)
    int16_t y[16][2];      // x, y
    int16_t c[4][2];
};
static_assert(sizeof(Vp8SplitMv) == 80, "Vp8SplitMv is 80 bytes");

struct Vp8PicParams {
    uint8_t *surf;                // the NV12 surface the picture is decoded into
    int pitch, chroma_offset;
    int mb_w, mb_h;               // macroblocks per row / rows; the surface holds 16 mb_w x 16 mb_h luma samples, nothing is read or stored beyond them.
                                  // mb_w == 0: the picture takes no part
    int n_entries;
    int filter_type;              // 0 normal, 1 simple (luma only)
    int sharpness;                // 0..7
    int filtered;                 // some macroblock has a non-zero level (else k_vp8_filter has nothing to do for the picture)
    const Vp8Mb *mbs;             // [mb_w * mb_h]
    const uint32_t *entries;      // [n_entries]
    int16_t dq[4][6];             // per segment: y1 dc, y1 ac, y2 dc, y2 ac, uv dc, uv ac (the RFC's clamps and the y2 / uv rules applied)
    // option vp8_inter.  All zero: a key frame, every macroblock intra
    int inter;                    // 1: an inter frame -- k_vp8_inter predicts its VP8_MB_INTER macroblocks, the loop filter takes the inter hev thresholds
    int interp;                   // 0 six-tap (version 0), 1 bilinear (versions 1 .. 3)
    int n_intra;                  // inter frame: its intra macroblocks (0: k_vp8_recon has nothing to do for the picture)
    int n_split;
    const uint8_t *ref[3];        // last, golden, altref: finished (loop-filtered) surfaces of the same geometry; never the surface being decoded
    const Vp8SplitMv *split;      // [n_split]
};

// one wave per macroblock, blockIdx.y = picture; max_mbs: the most macroblocks of a picture of the batch.  Pictures with inter == 0 take no part
void launch_vp8_inter(const Vp8PicParams *d_pics, int n, int max_mbs, ihipStream_t *st);
// blockIdx.x = picture, one workgroup per picture; a picture with mb_w == 0 takes no part.  any_inter: some picture of the batch is an inter frame -- without
// one the kernels compiled without the inter tests run, which are the key-frame kernels as they were before the option
void launch_vp8_recon(const Vp8PicParams *d_pics, int n, bool any_inter, ihipStream_t *st);
void launch_vp8_filter(const Vp8PicParams *d_pics, int n, bool any_inter, ihipStream_t *st);

}  // namespace jmamd
