// jmcodec_amd/csrc/hevc_kernels.h -- host-callable launcher of the HEVC kernels (hevc_kernels.hip); one call = one batch of pictures.
#pragma once
#include <hip/hip_runtime_api.h>
#include "hevc_jobs.h"

namespace jmamd {
struct HevcBatchDims { int max_pus = 0, max_tbs = 0, max_itbs = 0, max_ctb_w = 0, max_ctb_h = 0, max_w = 0, max_h = 0;
    bool any_intra = false, any_deblock = false, any_sao = false;
    bool any_hash = false,           // some picture asks for its CRC / checksum (HevcPicParams::hash_mode bit 0): k_hevc_pichash runs behind the last filter
         any_md5 = false; };         // ... for its MD5 (bit 1): k_hevc_md5 runs behind that
// marks (optional, 4 events): before MC, after residual, after intra, after the loop filters
constexpr int kHevcIntraSegs = 8;             // workgroups per CTB row in k_hevc_intra (each walks a run of consecutive CTBs)
constexpr int kHevcProgressStride = 544 * kHevcIntraSegs;   // progress counters per picture: one per CTB row (8192 / 16 + slack) and segment
// progress: device array of n * kHevcProgressStride ints (row progress counters of k_hevc_intra, cleared by this call)
// hash: the batch's result words (kHashStride per picture), needed when m.any_hash; marks then has a fifth event, recorded behind k_hevc_pichash
void launch_hevc_picture_batch(const HevcPicParams *d_pics, int n, const HevcBatchDims &m, int *progress, hipStream_t st, hipEvent_t *marks, uint32_t *hash);
// k_hevc_pichash (pichash.hip) alone: clears n * kHashStride words of d_hash on st, then per picture with bit 0 of hash_mode words 0..2 = the CRC of Y, Cb, Cr
// of surf[cur] (coded size w x h), words 3..5 = their checksums (INTEGRATION.md "Picture hash")
constexpr int kHashStride = 32;               // words per picture: the six results and padding to a cache line of their own (they are atomics' targets)
void launch_hevc_pichash(const HevcPicParams *d_pics, int n, int max_h, uint32_t *d_hash, hipStream_t st);
// k_hevc_md5 (pichash.hip) alone: per picture with bit 1 of hash_mode, words kMd5Word + 4 c .. + 3 = the MD5 of component c (Y, Cb, Cr) of surf[cur], the
// digest's 16 bytes in RFC 1321 order when the words lie in memory least significant byte first.  Plain stores: nothing needs clearing
constexpr int kMd5Word = 8;
static_assert(kMd5Word >= 6 && kMd5Word + 12 <= kHashStride, "the digests lie behind the six CRC / checksum words of a picture");
void launch_hevc_md5(const HevcPicParams *d_pics, int n, uint32_t *d_hash, hipStream_t st);
void hevc_kernels_init();
}  // namespace jmamd
