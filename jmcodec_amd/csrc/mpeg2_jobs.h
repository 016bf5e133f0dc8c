// jmcodec_amd/csrc/mpeg2_jobs.h -- what the host hands k_mpeg2_recon for one MPEG-2 picture, a frame picture or (option mpeg2_field_pictures) one
// field picture (codec_type 4; INTEGRATION.md "MPEG-2").
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
    M2_16X8 = 64,          // field pictures only: 16x8 motion compensation, vectors 0 / 1 of a direction predict lines 0..7 / 8..15 of the macroblock
    M2_DUAL = 128,         // dual prime (P pictures, M2_FWD alone): the host has derived the opposite-parity vectors, the device fetches and averages
    M2_SEL_SHIFT = 8       // bits 8..11: motion_vertical_field_select of vectors fwd 0, fwd 1, bwd 0, bwd 1
};
// Which mv[] slot holds what (slot 2 s + r: direction s, vector r; every field vector's y counts lines of its field):
//   frame picture, frame prediction            slot 2 s
//   frame picture, M2_FIELD_MV                 slot 2 s + r for the lines of parity r, from the field select bit 2 s + r names
//   frame picture, M2_DUAL                     slot 0 = the transmitted vector v (field format): top lines from the top field, bottom lines from the bottom field;
//                                              slot 2 = the derived vector for the top lines (read from the bottom field), slot 3 = the derived vector for the
//                                              bottom lines (read from the top field); slot 1 is unused
//   field picture, field prediction            slot 2 s, from the field select bit 2 s names (M2_FIELD_MV is not set: every prediction of a field picture
//                                              reads a field)
//   field picture, M2_16X8                     slot 2 s + r for lines 8 r .. 8 r + 7 of the field macroblock, from the field select bit 2 s + r names
//   field picture, M2_DUAL                     slot 0 = v, read from the field of the picture's own parity; slot 2 = the derived vector, read from the
//                                              opposite parity; slots 1 and 3 are unused
// A dual-prime macroblock is forward only, so its backward slots are free for the derived vectors; the two fetches are averaged (a + b + 1) >> 1.

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
    // ---- option mpeg2_field_pictures; all zero: a frame picture without 16x8 or dual-prime records, as before the option existed ----
    int structure;                // 0 a frame picture; 1 / 2 a top / bottom field picture: mb_h counts the FIELD's macroblock rows, a field's line y is
                                  // surface line 2 y + structure - 1 (luma and interleaved chroma alike), nothing of the other parity is stored
    int ext;                      // the picture needs the kernel that knows field pictures, 16x8 and dual prime (structure != 0, or a record says so)
    const uint8_t *fref[2][2];    // field pictures: [direction][parity] -> the first luma sample of that reference field, lines 2 pitch apart (its chroma:
                                  // + chroma_offset); nullptr: none -- the prediction reads 128.  (The picture that fills in the missing field of a lone anchor field names the existing field for both)
};

// blockIdx.y = picture; a picture with n_items == 0 takes no part.  max_items: the largest n_items of the batch.  ext: some picture of the batch has
// Mpeg2PicParams::ext set -- the launch then runs the instantiation with the field-picture modes, else the one frame pictures always ran
void launch_mpeg2_recon(const Mpeg2PicParams *d_pics, int n, int max_items, bool ext, ihipStream_t *st);

// Option mpeg2_device_vlc: a picture whose slices the device VLC-decodes (k_mpeg2_vlc, in front of k_mpeg2_recon on the same stream).  The host
// uploads the picture's parameters, a slice table and the slice bytes (mpeg2_vlc.h); the records and entries -- the arrays Mpeg2PicParams names too --
// exist in device memory only and are written here.  tab: the engine's copy of the lookup tables, set by Engine::launch, as is status: kMpeg2StatusWords
// words of the batch's status array, zeroed before the launch: [0] counts the picture's damaged slices, [1] collects the kinds of damage (1 << kind,
// mpeg2_vlc.h), [2] counts the macroblocks whose vectors were clamped, [3] bit 0: holes were concealed, bit 1: dual prime was met
// and not allowed, bits 8..: dual-prime records written (option mpeg2_field_pictures).
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
