// jmcodec_amd/csrc/jpeg_jobs.h -- what the host hands k_jpeg_recon for one MJPEG picture (codec_type 2; INTEGRATION.md "MJPEG").
//
// The job list is SPARSE: per 8x8 block the index of its first entry and the number of its entries, and one 32-bit entry per non-zero level
// (zig-zag position | level << 16, levels saturated to int16 -- which leaves clip(level * Q) unchanged for every Q).  Blocks are indexed in plane
// raster order: the luma plane's y_bw x y_bh blocks, then Cb's c_bw x c_bh, then Cr's.  Quantisation tables travel here; the device dequantises.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

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

}  // namespace jmamd
