// jmcodec_amd/csrc/vp8_kernels.hip -- k_vp8_recon and k_vp8_filter: VP8 frames (codec_type 5) from their job lists into NV12 surfaces, gfx950; and
// k_vp8_inter (option vp8_inter; described where it stands, below): the inter macroblocks of inter frames, ahead of the other two.
//
// Both kernels walk a picture's macroblocks as a wavefront.  Reconstruction: a macroblock's intra prediction reads the UNFILTERED samples of its
// left, above and above-right neighbours.  Loop filter (RFC 6386 section 15: macroblocks in raster order, each filter reading what earlier ones
// wrote): macroblock (x, y) reads and writes up to 4 samples into (x - 1, y) and (x, y - 1), whose right columns (x + 1, y - 1)'s left-edge filter
// must have finished with.  Both orders are met by step s = x + 2 y: (x - 1, y) is step s - 1, (x, y - 1) step s - 2, (x + 1, y - 1) step s - 1.
//
// One workgroup per picture (blockIdx.x = picture, a batch's pictures side by side), 16 waves, one macroblock per wave and step.  The picture's rows
// are taken in bands of 16; in a band wave w owns row 16 band + w and at step s reconstructs (filters) macroblock x = s - 2 w of it, if there is one.
// The steps of a band are separated by __syncthreads(), which also makes a wave's global stores visible to the workgroup's other waves (they share
// the CU's vector L1); the last row of a band is complete when the band's loop ends, before the first row of the next band begins.
// Every barrier is reached by every wave of the workgroup: the band and step loops are bounded by mb_w and mb_h alone -- values of the picture's
// parameters, the same for all waves -- the test whether a wave has a macroblock at a step encloses no barrier, and the only early return is taken
// by a whole workgroup before the first barrier.  Nothing spins on memory and nothing waits for another workgroup, so no job list, however
// damaged, can stall a kernel; what a record can index is clamped where it is used (vp8_recon.h) after the host has validated it.
// Inside a step a wave works alone on its own LDS work area; the phases of a macroblock (vp8_recon.h says which lanes do what) are separated by a
// wave-level barrier: LDS operations of one wave execute in order, the barrier only keeps the compiler from moving them across.
//
// The filter runs as a second launch, after the whole batch's reconstruction: no prediction can see a filtered sample.  A picture whose macroblocks
// all have level 0 leaves it at once.
//
// LDS: k_vp8_recon 16 x sizeof(Vp8Work) = 16 x 2,984 = 47,744 bytes; k_vp8_filter 16 x 688 = 11,008 bytes.  The work areas are addressed byte-wise
// (ds_read_u8 / ds_write_b8) except for the dword copies of the filter's area and the zeroing; bank conflicts have not been worked out or measured:
// a step is supposed to be bound by its global round trip (borders in, macroblock out) and the barrier, not by LDS cycles -- a supposition from the
// structure, not a counter; the measured times per picture are in profiles/r22_vp8.txt.  No MFMA: 4x4 integer transforms.
// gfx950 compile (-Rpass-analysis=kernel-resource-usage), read from the compiler, not measured:
//   k_vp8_recon   (<true> and <false> alike) 85 VGPRs, 106 SGPRs (8 spilled to vector lanes), no scratch, 47,744 bytes of LDS, 5 waves per SIMD by the compiler's count
//                 (a workgroup is 16 waves = 4 per SIMD, and LDS lets 3 workgroups share a CU)
//   k_vp8_filter  63 VGPRs, 52 SGPRs, no scratch, 11,008 bytes of LDS, 8 waves per SIMD
//   k_vp8_inter   30 VGPRs, 41 SGPRs, no scratch, 4 x sizeof(Vp8InterWork) = 4 x 5,896 = 23,584 bytes of LDS, 6 waves per SIMD (LDS: 6 workgroups per CU)
#include <hip/hip_runtime.h>
#include "vp8_jobs.h"
#include "vp8_recon.h"

namespace jmamd {

constexpr int kVp8Waves = 16;

__device__ __forceinline__ void vp8_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// INTER: the batch holds an inter frame (option vp8_inter).  A batch of key frames runs the <false> kernels: the instruction path of before the option
template <bool INTER>
__device__ __forceinline__ void vp8_recon_mb(const Vp8PicParams &pp, Vp8Work &w, int mbx, int mby, int lane) {
    const Vp8Mb *rec = pp.mbs + (size_t)mby * pp.mb_w + mbx;
    const uint4 m0 = reinterpret_cast<const uint4 *>(rec)[0], m1 = reinterpret_cast<const uint4 *>(rec)[1];
    Vp8Mb mb;
    mb.first = m0.x; mb.count = (uint16_t)(m0.y & 0xffff); mb.ymode = (uint8_t)(m0.y >> 16); mb.uvmode = (uint8_t)(m0.y >> 24);
    mb.segment = (uint8_t)m0.z; mb.level = (uint8_t)(m0.z >> 8); mb.flags = (uint8_t)(m0.z >> 16); mb.mvmode = 0; mb.nz = m0.w;
    if (INTER && (mb.flags & VP8_MB_INTER)) return;                     // (wave-uniform; k_vp8_inter has put the macroblock on the surface)
    const bool bpred = mb.ymode >= VP8_B_PRED;
    vp8_zero_lane(w, lane);
    vp8_wave_sync();
    vp8_scatter_lane(w, mb, pp.entries, pp.n_entries, pp.dq[mb.segment & 3], lane);
    vp8_wave_sync();
    if (!bpred && (mb.nz >> 24 & 1)) { vp8_wht_lane(w, lane); vp8_wave_sync(); }
    vp8_idct_lane(w, mb, lane);
    vp8_borders_lane(w, pp.surf, pp.pitch, pp.chroma_offset, mbx, mby, pp.mb_w, lane);
    vp8_wave_sync();
    if (!bpred) vp8_luma16_lane(w, mb, mbx, mby, lane);
    else {
#pragma unroll 1
        for (int k = 0; k < 16; k++) {
            // the 16 sub-block modes are the record's last 16 bytes: m1.x .. m1.w, four each
            const uint32_t word = k < 8 ? (k < 4 ? m1.x : m1.y) : (k < 12 ? m1.z : m1.w);
            vp8_bpred_lane(w, (int)(word >> ((k & 3) * 8) & 0xff), k, lane);
            vp8_wave_sync();
        }
    }
    const uint32_t uv = vp8_chroma_lane(w, mb, mbx, mby, lane);
    vp8_wave_sync();
    vp8_store_lane(w, pp.surf, pp.pitch, pp.chroma_offset, mbx, mby, uv, lane);
}

template <bool INTER>
__global__ __launch_bounds__(64 * kVp8Waves) void k_vp8_recon(const Vp8PicParams *pics) {
    const Vp8PicParams &pp = pics[blockIdx.x];
    if (pp.mb_w <= 0 || pp.mb_h <= 0 || (INTER && pp.inter && pp.n_intra == 0)) return;      // (the whole workgroup: no barrier is left behind)
    __shared__ __attribute__((aligned(16))) Vp8Work sW[kVp8Waves];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int mb_w = pp.mb_w, mb_h = pp.mb_h;
    for (int row0 = 0; row0 < mb_h; row0 += kVp8Waves) {
        const int rows = mb_h - row0 < kVp8Waves ? mb_h - row0 : kVp8Waves;
        const int n_steps = mb_w + 2 * (rows - 1);
        const int mby = row0 + wave;
#pragma unroll 1
        for (int s = 0; s < n_steps; s++) {
            const int mbx = s - 2 * wave;
            if (wave < rows && mbx >= 0 && mbx < mb_w) vp8_recon_mb<INTER>(pp, sW[wave], mbx, mby, lane);
            __syncthreads();
        }
    }
}

template <bool INTER>
__device__ __forceinline__ void vp8_filter_mb(const Vp8PicParams &pp, Vp8FiltWork &w, int mbx, int mby, int lane) {
    const Vp8Mb *rec = pp.mbs + (size_t)mby * pp.mb_w + mbx;
    const uint4 m0 = reinterpret_cast<const uint4 *>(rec)[0];
    Vp8Mb mb = {};
    mb.level = (uint8_t)(m0.z >> 8); mb.flags = (uint8_t)(m0.z >> 16);
    if (!mb.level) return;                                              // (wave-uniform; no barrier below but wave-level ones)
    vp8_filt_copy_lane(w, pp.surf, pp.pitch, pp.chroma_offset, mbx, mby, false, lane);
    vp8_wave_sync();
    vp8_filter_lane(w, mb, pp.filter_type, pp.sharpness, mbx, mby, 0, lane, INTER ? pp.inter : 0);
    vp8_wave_sync();
    vp8_filter_lane(w, mb, pp.filter_type, pp.sharpness, mbx, mby, 1, lane, INTER ? pp.inter : 0);
    vp8_wave_sync();
    vp8_filt_copy_lane(w, pp.surf, pp.pitch, pp.chroma_offset, mbx, mby, true, lane);
}

template <bool INTER>
__global__ __launch_bounds__(64 * kVp8Waves) void k_vp8_filter(const Vp8PicParams *pics) {
    const Vp8PicParams &pp = pics[blockIdx.x];
    if (pp.mb_w <= 0 || pp.mb_h <= 0 || !pp.filtered) return;         // (the whole workgroup: no barrier is left behind)
    __shared__ __attribute__((aligned(16))) Vp8FiltWork sW[kVp8Waves];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int mb_w = pp.mb_w, mb_h = pp.mb_h;
    for (int row0 = 0; row0 < mb_h; row0 += kVp8Waves) {
        const int rows = mb_h - row0 < kVp8Waves ? mb_h - row0 : kVp8Waves;
        const int n_steps = mb_w + 2 * (rows - 1);
        const int mby = row0 + wave;
#pragma unroll 1
        for (int s = 0; s < n_steps; s++) {
            const int mbx = s - 2 * wave;
            if (wave < rows && mbx >= 0 && mbx < mb_w) vp8_filter_mb<INTER>(pp, sW[wave], mbx, mby, lane);
            __syncthreads();
        }
    }
}

// k_vp8_inter (option vp8_inter): the inter macroblocks of the batch's inter frames, one wave per macroblock, kVp8InterWaves macroblocks per workgroup,
// blockIdx.y = picture.  The pictures of a batch reference only surfaces that earlier launches on this in-order stream finished (Engine::form), and
// a macroblock reads the references and writes its own 16 x 16 of the current surface -- never a reference: no macroblock waits for another, there
// is no workgroup barrier and nothing spins.  A wave works alone on its Vp8InterWork; the phases are separated by wave-level barriers as above.
// Per macroblock (derived from the code, not measured): 779 window bytes (SPLITMV: 1,944) fetched as BYTE loads with clamped coordinates -- 13 (31) loads
// per lane; dword loads where a window row is aligned and inside the area are the next step, as k_mpeg2_recon took it -- then 544 (864) first-pass and
// 384 second-pass samples of six multiply-adds each from LDS bytes, 8.5 (13.5) + 6 per lane, and one dword + one 16-bit store per lane.  Like
// k_mpeg2_recon and k_hevc_mc it is supposed to be bound by instruction issue (byte loads, LDS byte reads), not by memory: 1.2 KB in and 384 bytes out
// per macroblock.  The tap rows come from a switch, not a table in memory.  Measured times: profiles/r23_vp8_inter.txt.
constexpr int kVp8InterWaves = 4;

__global__ __launch_bounds__(64 * kVp8InterWaves) void k_vp8_inter(const Vp8PicParams *pics) {
    const Vp8PicParams &pp = pics[blockIdx.y];
    if (pp.mb_w <= 0 || pp.mb_h <= 0 || !pp.inter) return;
    __shared__ __attribute__((aligned(16))) Vp8InterWork sW[kVp8InterWaves];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int mbi = (int)blockIdx.x * kVp8InterWaves + wave;
    if (mbi >= pp.mb_w * pp.mb_h) return;                               // (wave-uniform, as every return below: the record is the wave's)
    const int mby = mbi / pp.mb_w, mbx = mbi - mby * pp.mb_w;
    const Vp8Mb *rec = pp.mbs + mbi;
    const uint4 m0 = reinterpret_cast<const uint4 *>(rec)[0], m1 = reinterpret_cast<const uint4 *>(rec)[1];
    Vp8Mb mb;
    mb.first = m0.x; mb.count = (uint16_t)(m0.y & 0xffff); mb.ymode = (uint8_t)(m0.y >> 16); mb.uvmode = (uint8_t)(m0.y >> 24);
    mb.segment = (uint8_t)m0.z; mb.level = (uint8_t)(m0.z >> 8); mb.flags = (uint8_t)(m0.z >> 16); mb.mvmode = (uint8_t)(m0.z >> 24); mb.nz = m0.w;
    if (!(mb.flags & VP8_MB_INTER)) return;
    const uint32_t words[4] = {m1.x, m1.y, m1.z, m1.w};
    Vp8InterInfo ii; const uint8_t *ref; const Vp8SplitMv *sv;
    if (!vp8_inter_info(pp, words, ii, ref, sv)) return;
    Vp8InterWork &iw = sW[wave];
    const bool split = sv != nullptr, has_res = mb.count != 0;
    vp8_inter_mvs_lane(iw, ii, sv, lane);
    if (has_res) {
        vp8_zero_lane(iw.w, lane);
        vp8_wave_sync();
        vp8_scatter_lane(iw.w, mb, pp.entries, pp.n_entries, pp.dq[mb.segment & 3], lane);
        vp8_wave_sync();
        if (mb.ymode != VP8_B_PRED && (mb.nz >> 24 & 1)) { vp8_wht_lane(iw.w, lane); vp8_wave_sync(); }
        vp8_idct_lane(iw.w, mb, lane);
    }
    vp8_wave_sync();
    vp8_inter_fetch_lane(iw, split, ref, pp.pitch, pp.chroma_offset, pp.mb_w, pp.mb_h, mbx, mby, lane);
    vp8_wave_sync();
    vp8_inter_hpass_lane(iw, split, pp.interp, lane);
    vp8_wave_sync();
    vp8_inter_vpass_lane(iw, split, pp.interp, has_res, lane);
    vp8_wave_sync();
    vp8_inter_store_lane(iw, pp.surf, pp.pitch, pp.chroma_offset, mbx, mby, lane);
}

void launch_vp8_inter(const Vp8PicParams *d_pics, int n, int max_mbs, ihipStream_t *st) {
    if (n <= 0 || max_mbs <= 0) return;
    hipLaunchKernelGGL(k_vp8_inter, dim3((max_mbs + kVp8InterWaves - 1) / kVp8InterWaves, n), dim3(64 * kVp8InterWaves), 0, st, d_pics);
}
void launch_vp8_recon(const Vp8PicParams *d_pics, int n, bool any_inter, ihipStream_t *st) {
    if (n <= 0) return;
    if (any_inter) hipLaunchKernelGGL(k_vp8_recon<true>, dim3(n), dim3(64 * kVp8Waves), 0, st, d_pics);
    else hipLaunchKernelGGL(k_vp8_recon<false>, dim3(n), dim3(64 * kVp8Waves), 0, st, d_pics);
}
void launch_vp8_filter(const Vp8PicParams *d_pics, int n, bool any_inter, ihipStream_t *st) {
    if (n <= 0) return;
    if (any_inter) hipLaunchKernelGGL(k_vp8_filter<true>, dim3(n), dim3(64 * kVp8Waves), 0, st, d_pics);
    else hipLaunchKernelGGL(k_vp8_filter<false>, dim3(n), dim3(64 * kVp8Waves), 0, st, d_pics);
}

}  // namespace jmamd
