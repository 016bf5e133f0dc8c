// jmcodec_amd/csrc/mpeg2_jobs.h -- what the host hands k_mpeg2_recon for one MPEG-2 frame picture (codec_type 4; INTEGRATION.md "MPEG-2").
//
// The host resolves the whole syntax: one fixed-size record per macroblock in raster order -- skipped, zero-vector and concealed macroblocks get
// ordinary records -- and a SPARSE entry list in the style of jpeg_jobs.h: one 32-bit entry per non-zero level, natural (raster) position v * 8 + u
// in bits 0..5 | QF level << 16, the scan already applied.  The entries of a macroblock are contiguous from `first`, block after block in the order
// Y0 Y1 Y2 Y3 Cb Cr, count[k] of them for block k.  The quantiser matrices travel in the picture's parameters; the device dequantises.
#pragma once
#include <stdint.h>

struct ihipStream_t;

namespace jmamd {

enum : uint16_t {
    M2_INTRA = 1, M2_FWD = 2, M2_BWD = 4,
    M2_FIELD_MV = 8,       // field prediction in a frame picture: vectors 0 / 1 of a direction predict the top / bottom lines, each from the field it selects
    M2_FIELD_DCT = 16,     // dct_type 1: the luma blocks hold the lines of one field each
    M2_CLAMPED = 32,       // a vector reached outside the reference picture and was clamped by the host (the picture counts in `errors`)
    M2_SEL_SHIFT = 8       // bits 8..11: motion_vertical_field_select of vectors fwd 0, fwd 1, bwd 0, bwd 1
};

struct Mpeg2Mb {           // 32 bytes
    uint16_t flags;
    uint8_t qscale;        // quantiser_scale (1..112), resolved through q_scale_type
    uint8_t cbp;           // coded block pattern, bit 5 = Y0 .. bit 0 = Cr (an intra macroblock: 63)
    int16_t mv[4][2];      // fwd 0, fwd 1, bwd 0, bwd 1: x, y in half samples, reconstructed; a field vector's y counts lines of its field
    uint32_t first;        // index of the macroblock's first entry
    uint8_t count[6];      // entries of blocks Y0 Y1 Y2 Y3 Cb Cr
    uint8_t pad[2];
};
static_assert(sizeof(Mpeg2Mb) == 32, "Mpeg2Mb is 32 bytes");

struct Mpeg2PicParams {
    uint8_t *surf;                // the NV12 surface the picture is decoded into
    const uint8_t *ref[2];        // forward / backward reference surfaces (nullptr: none -- the prediction reads 128)
    int pitch, chroma_offset;
    int mb_w, mb_h;               // macroblocks per row / rows; the surface holds 16 mb_w x 16 mb_h luma samples, nothing is read or stored beyond them
    int n_items;                  // work items (one wave each): strips of 4 neighbouring macroblocks of one macroblock row
    int n_entries;
    int dc_mult;                  // intra_dc_mult: 8, 4, 2, 1 for intra_dc_precision 8..11
    int pad;
    const Mpeg2Mb *mbs;           // [mb_w * mb_h]
    const uint32_t *entries;      // [n_entries]
    uint8_t w[2][64];             // intra / non-intra quantiser matrix in natural (raster) order
};

// blockIdx.y = picture; a picture with n_items == 0 takes no part.  max_items: the largest n_items of the batch
void launch_mpeg2_recon(const Mpeg2PicParams *d_pics, int n, int max_items, ihipStream_t *st);

// Option mpeg2_device_vlc: a picture whose slices the device VLC-decodes (k_mpeg2_vlc, in front of k_mpeg2_recon on the same stream).  The host
// uploads the picture's parameters, a slice table and the slice bytes (mpeg2_vlc.h); the records and entries -- the arrays Mpeg2PicParams names too --
// exist in device memory only and are written here.  tab: the engine's copy of the lookup tables, set by Engine::launch, as is status: kMpeg2StatusWords
// words of the batch's status array, zeroed before the launch: [0] counts the picture's damaged slices, [1] collects the kinds of damage (1 << kind,
// mpeg2_vlc.h), [2] counts the macroblocks whose vectors were clamped, [3] bit 0: holes were concealed, bit 1: dual prime was met.
struct Mpeg2VlcTables; struct Mpeg2VlcPic; struct Mpeg2Slice;
constexpr int kMpeg2StatusWords = 4;
struct Mpeg2VlcParams {
    int n_slices;                 // 0: the picture takes no part (host path, another codec, no picture)
    int pad;
    const Mpeg2VlcPic *pic;
    const Mpeg2Slice *slices;     // [n_slices]
    const uint32_t *bytes;
    const Mpeg2VlcTables *tab;
    Mpeg2Mb *mbs; uint32_t *entries;
    uint32_t *status;
};
// blockIdx.y = picture, one lane per slice, workgroups of 64 lanes.  max_slices: the largest n_slices of the batch
void launch_mpeg2_vlc(const Mpeg2VlcParams *d_pics, int n, int max_slices, ihipStream_t *st);

}  // namespace jmamd
