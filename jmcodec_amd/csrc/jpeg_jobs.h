// jmcodec_amd/csrc/jpeg_jobs.h -- what the host hands k_jpeg_recon for one MJPEG picture (codec_type 2; INTEGRATION.md "MJPEG").
//
// The job list is SPARSE: per 8x8 block the index of its first entry and the number of its entries, and one 32-bit entry per non-zero level
// (zig-zag position | level << 16, levels saturated to int16 -- which leaves clip(level * Q) unchanged for every Q).  Blocks are indexed in plane
// raster order: the luma plane's y_bw x y_bh blocks, then Cb's c_bw x c_bh, then Cr's.  Quantisation tables travel here; the device dequantises.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "jpeg_entropy.h"

namespace jmamd {

struct JpegPicParams {
    uint8_t *surf;                // the NV12 surface the picture is decoded into
    int pitch, chroma_offset;
    int coded_w, coded_h;         // luma samples the surface holds per row / rows (multiples of 16): nothing is stored beyond them
    int sampling;                 // 0x22 4:2:0, 0x21 4:2:2, 0x11 4:4:4, 0x10 grey (the surface's chroma stays 128)
    int y_bw, y_bh, c_bw, c_bh;   // blocks per row / rows of the luma plane and of one chroma plane (padded to whole MCUs)
    int n_items_y, n_items;       // work items (one wave each): luma strips of 8 blocks first, then chroma strips of 4 Cb + 4 Cr blocks
    int n_blocks, n_entries;
    const uint32_t *first;        // [n_blocks]
    const uint8_t *count;         // [n_blocks]
    const uint32_t *entries;      // [n_entries]
    uint8_t q[3][64];             // per component, in zig-zag order (as DQT carries them)
};

// blockIdx.y = picture; a picture with n_items == 0 takes no part.  max_items: the largest n_items of the batch
void launch_jpeg_recon(const JpegPicParams *d_pics, int n, int max_items, hipStream_t st);

// Option jpeg_device_entropy: a picture whose scan the device entropy-decodes (k_jpeg_entropy, in front of k_jpeg_recon on the same stream).  The
// host uploads tables, segment table and clean bytes (jpeg_entropy.h); first / count / entries -- the arrays JpegPicParams names too -- exist in
// device memory only and are written here.  status: two words of the batch's status array, zeroed before the launch: [0] counts the picture's
// damaged segments, [1] collects the kinds of damage (kJpegDamage*).
constexpr int kJpegStatusWords = 2;
struct JpegEntropyParams {
    int n_segs;                   // 0: the picture takes no part (host path, another codec, no picture)
    JpegScanGeom geom;
    const JpegDevHuff *tab;       // [6]
    const JpegSegment *segs;      // [n_segs]
    const uint32_t *bytes;
    uint32_t *first; uint8_t *count; uint32_t *entries;
    uint32_t *status;
};
// blockIdx.y = picture, one lane per segment.  max_segs: the largest n_segs of the batch
void launch_jpeg_entropy(const JpegEntropyParams *d_pics, int n, int max_segs, hipStream_t st);

}  // namespace jmamd
