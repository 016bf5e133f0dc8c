// tools/fuzz_stubs.h -- stand-ins for the kernel launchers (never reached in parse-only mode), so that the host sources link without the device objects;
// included by the sanitizer harnesses (fuzz_host.cpp, fuzz_pushpull.cpp) and by host_bench.cpp
#pragma once
#include <cstdlib>
#include "../jmcodec_amd/csrc/kernels.h"
namespace jmamd {
bool deblock_lds_supported(int, int) { return true; }
bool intra_lds_supported(int, int) { return true; }
void launch_packout(const PackJob *, int, int, int, ihipStream_t *) { abort(); }
int scale_tiles(int, int) { return 1; }
void launch_scale_pack(const ScaleJob *, int, int, ihipStream_t *) { abort(); }
int rgb_tiles(int, int) { return 1; }
void launch_rgb_pack(const RgbJob *, int, int, int, int, ihipStream_t *) { abort(); }
int deint_items(int, int) { return 1; }
void launch_deint(const DeintJob *, int, int, ihipStream_t *) { abort(); }
int deint2_items(int, int) { return 1; }
void launch_deint2(const DeintJob *, int, int, ihipStream_t *) { abort(); }
void launch_deint3(const DeintJob *, int, int, ihipStream_t *) { abort(); }
void launch_recon_inter(const PicParams *, int, int, bool, bool, int *, ihipStream_t *) { abort(); }
void launch_intra_lds(const PicParams *, int, int, int *, int *, ihipStream_t *) { abort(); }
void launch_recon_intra(const PicParams *, int, ihipStream_t *) { abort(); }
void launch_deblock_prep(const PicParams *, int, int, ihipStream_t *) { abort(); }
void launch_deblock_lds(const PicParams *, int, int, int *, int *, bool, ihipStream_t *) { abort(); }
bool chain_supported(int, int) { return true; }
int chain_ctl_ints() { return 1; }
int chain_tail_ints() { return 32; }
int chain_tail_head_ints() { return 32; }
int chain_tail_wait_limit() { return 15; }
void launch_chain(const PicParams *, const uint32_t *, int, bool, int *, int *, bool, ihipStream_t *) { abort(); }
int chain_band_rows() { return 16; }
int deblock_row_lag() { return 1; }
int chain_resident_workgroups(bool) { return 0; }
void launch_deblock(const PicParams *, int, ihipStream_t *) { abort(); }
}
namespace jmamd { void launch_frame_to_argb(const uint8_t *, int, int, int, uint8_t *, int, ihipStream_t *) { abort(); }
void launch_frame_to_nv12_pitch(const uint8_t *, int, int, int, uint8_t *, int, ihipStream_t *) { abort(); } }
#include "../jmcodec_amd/csrc/hevc_kernels.h"
#include "../jmcodec_amd/csrc/jpeg_jobs.h"
#include "../jmcodec_amd/csrc/mpeg2_jobs.h"
#include "../jmcodec_amd/csrc/vp8_jobs.h"
namespace jmamd {
void launch_hevc_picture_batch(const HevcPicParams *, int, const HevcBatchDims &, int *, ihipStream_t *, ihipEvent_t **, uint32_t *) { abort(); }
void launch_hevc_pichash(const HevcPicParams *, int, int, uint32_t *, ihipStream_t *) { abort(); }
void launch_hevc_md5(const HevcPicParams *, int, uint32_t *, ihipStream_t *) { abort(); }
void launch_jpeg_recon(const JpegPicParams *, int, int, ihipStream_t *) { abort(); }
void launch_jpeg_entropy(const JpegEntropyParams *, int, int, ihipStream_t *) { abort(); }
void launch_mpeg2_recon(const Mpeg2PicParams *, int, int, bool, ihipStream_t *) { abort(); }
void launch_mpeg2_vlc(const Mpeg2VlcParams *, int, int, ihipStream_t *) { abort(); }
void launch_vp8_inter(const Vp8PicParams *, int, int, ihipStream_t *) { abort(); }
void launch_vp8_recon(const Vp8PicParams *, int, bool, ihipStream_t *) { abort(); }
void launch_vp8_filter(const Vp8PicParams *, int, bool, ihipStream_t *) { abort(); }
void hevc_kernels_init() {}
}
