// jmcodec_amd/csrc/vp8_jobs.h -- what the host hands k_vp8_recon and k_vp8_filter for one VP8 key frame (codec_type 5; INTEGRATION.md "VP8").
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
    VP8_MB_INNER = 1       // the loop filter also filters the macroblock's inner edges: B_PRED, or some block has coefficients (RFC 6386 15.1... 15.3)
};
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
    uint8_t pad;
    uint32_t nz;           // bit b: block b (numbered as in the entries) has at least one entry
    uint8_t bmodes[16];    // B_PRED: the sub-block modes in raster order (else the implied modes; the device does not read them then)
};
static_assert(sizeof(Vp8Mb) == 32, "Vp8Mb is 32 bytes");

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
};

// blockIdx.x = picture, one workgroup per picture; a picture with mb_w == 0 takes no part
void launch_vp8_recon(const Vp8PicParams *d_pics, int n, ihipStream_t *st);
void launch_vp8_filter(const Vp8PicParams *d_pics, int n, ihipStream_t *st);

}  // namespace jmamd
