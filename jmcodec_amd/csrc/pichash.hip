// jmcodec_amd/csrc/pichash.hip -- k_hevc_pichash: the CRC and the checksum of the decoded picture hash SEI (H.265 D.3.19) of every picture of a batch
// that asks for them, from the finished surface (INTEGRATION.md "Picture hash"; the arithmetic is pichash_packed.h, which the host walks too).
//
// grid (bands, pictures): a workgroup reads kBandRows luma rows and the chroma rows below them ONCE, 16 bytes per lane and load, and computes both
// hashes of all three components from that read.  Both hashes are sums -- mod 2^32, and over GF(2) once every lane has moved its piece of the CRC to
// its place in the picture (pichash_packed.h) -- so a workgroup reduces its lanes (ds_bpermute inside a wave, an LDS array across the four waves) and
// adds ONE value per result word with a device-scope atomicAdd / atomicXor.  Integer add and xor do not depend on the order of arrival: the words are
// the same in every run, without a slab of partial results and a second pass.  The caller clears the words in front of the launch.
// k_hevc_md5, further down: the MD5 of the same message (hash_type 0, option verify_md5) -- one serial chain per component; md5_packed.h.
// There is no reference counterpart: the reference's decoder never looks at SEI (/root/reference/nv_dec/nv_dec.cpp:368-403 hands the bytes to cuvid).
#include <hip/hip_runtime.h>
#include <mutex>
#include "hevc_kernels.h"
#include "pichash_packed.h"
#include "md5_packed.h"

namespace jmamd {

__device__ uint16_t g_pichash_pow[ph::kPowLo + ph::kPowHi];      // x^i, i < 256, then x^(256 i), i < 128 (mod P)

__global__ __launch_bounds__(256) void k_hevc_pichash(const HevcPicParams *pics, uint32_t *hash) {
    const HevcPicParams &pp = pics[blockIdx.y];
    if (!(pp.hash_mode & 1)) return;
    const int w = pp.w, h = pp.h, band = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (band >= ph::band_count(h)) return;
    __shared__ uint16_t pw[ph::kPowLo + ph::kPowHi];
    __shared__ uint32_t part[4][6];
    for (int i = tid; i < ph::kPowLo + ph::kPowHi; i += 256) pw[i] = g_pichash_pow[i];
    __syncthreads();
    const uint16_t *lo = pw, *hi = pw + ph::kPowLo;
    const ph::sbyte *surf = (const ph::sbyte *)pp.surf[pp.cur];
    const bool wide = (((uintptr_t)surf | (uintptr_t)pp.pitch | (uintptr_t)pp.chroma_offset) & 15) == 0;
    ph::Acc a;
    const int items = ph::band_items(w, h, band);
    for (int i = tid; i < items; i += 256) ph::hash_item(surf, pp.pitch, pp.chroma_offset, w, h, band, i, wide, lo, hi, a);
    uint32_t v[6] = {a.crc_y, a.crc_cb, a.crc_cr, a.sum_y, a.sum_cb, a.sum_cr};
    // the initial value's term, once per component
    if (band == 0 && tid == 0) {
        const uint32_t cbytes = (uint32_t)(w >> 1) * (uint32_t)(h >> 1);
        v[0] ^= ph::init_term((uint32_t)w * (uint32_t)h, lo, hi); v[1] ^= ph::init_term(cbytes, lo, hi); v[2] ^= ph::init_term(cbytes, lo, hi);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; k++) { v[k] ^= (uint32_t)__shfl_xor((int)v[k], off, 64); v[3 + k] += (uint32_t)__shfl_xor((int)v[3 + k], off, 64); }
    }
    if ((tid & 63) == 0) for (int k = 0; k < 6; k++) part[tid >> 6][k] = v[k];
    __syncthreads();
    if (tid < 6) {
        uint32_t *out = hash + (size_t)blockIdx.y * kHashStride + tid;
        if (tid < 3) atomicXor(out, part[0][tid] ^ part[1][tid] ^ part[2][tid] ^ part[3][tid]);
        else atomicAdd(out, part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid]);
    }
}

static bool upload_pow_tables() {
    static std::mutex m; static bool done[64] = {false};
    std::lock_guard<std::mutex> lk(m);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (done[dev]) return true;
    uint16_t t[ph::kPowLo + ph::kPowHi];
    ph::fill_pow_tables(t, t + ph::kPowLo);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_pichash_pow), t, sizeof t) != hipSuccess) return false;
    return done[dev] = true;
}

// k_hevc_md5: the MD5 of Y, Cb and Cr of every picture of the batch whose hash_mode has bit 1 (md5_packed.h has the arithmetic and the stream's layout).
// grid (3 components, pictures), one workgroup of 256 per chain; no workgroup talks to another and there are no atomics.
// An MD5 chain is serial -- 64 steps per 64-byte block, every one waiting for the last -- so the kernel's time IS the chain's latency, and the one thing
// to arrange is that the chain never waits for memory.  Wave 0 runs the chain; waves 1..3 stage the NEXT tile of the component's padded byte stream
// (rows gathered at the pitch, chroma de-interleaved, the RFC's padding written in) into the other half of an LDS double buffer meanwhile, so wave 0
// only ever sees whole blocks in LDS.  One barrier per tile; the number of tiles depends on w, h and the component only, so every wave meets every
// barrier.  All 64 lanes of wave 0 compute the SAME chain from the same LDS words (identical addresses broadcast): a vector instruction costs one lane
// what it costs sixty-four, so the redundancy is free, and spreading one chain over lanes is impossible anyway.  Lane 0 stores the four state words
// -- the digest's 16 bytes in RFC order on this little-endian machine -- with plain vector stores.
__global__ __launch_bounds__(256) void k_hevc_md5(const HevcPicParams *pics, uint32_t *hash) {
    const HevcPicParams &pp = pics[blockIdx.y];
    if (!(pp.hash_mode & 2)) return;
    __shared__ uint4 tile[2][md5::kTileWords / 4];
    const int w = pp.w, h = pp.h, c = (int)blockIdx.x, tid = (int)threadIdx.x;
    const ph::sbyte *surf = (const ph::sbyte *)pp.surf[pp.cur];
    const bool wide = (((uintptr_t)surf | (uintptr_t)pp.pitch | (uintptr_t)pp.chroma_offset) & 15) == 0;
    const uint32_t n = md5::comp_bytes(w, h, c);
    const int tiles = md5::tile_count(n);
    auto stage = [&](int t, int first, int step) {
        const int items = md5::tile_items(n, t);
        for (int i = first; i < items; i += step) {
            uint32_t v[4];
            md5::stage_item(surf, pp.pitch, pp.chroma_offset, w, h, c, t, i, wide, v);
            tile[t & 1][i] = make_uint4(v[0], v[1], v[2], v[3]);
        }
    };
    stage(0, tid, 256);                                  // the first tile: everyone
    __syncthreads();
    uint32_t state[4] = {md5::kInit[0], md5::kInit[1], md5::kInit[2], md5::kInit[3]};
    for (int t = 0; t < tiles; t++) {
        if (tid >= 64) { if (t + 1 < tiles) stage(t + 1, tid - 64, 192); }
        else {
            const uint4 *blk = tile[t & 1];
            const int blocks = md5::tile_blocks(n, t);
            // every lane reads the same words, so they are held in scalar registers: M[g] + K[i] is then scalar arithmetic beside the chain
            auto first = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
            uint32_t m[16];
            { const uint4 q0 = blk[0], q1 = blk[1], q2 = blk[2], q3 = blk[3];
              const uint32_t v[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
              for (int k = 0; k < 16; k++) m[k] = first(v[k]); }
            for (int b = 0; b < blocks; b++) {
                // the next block's words are fetched while this block's 64 steps run (the tile's last block fetches itself again: no branch)
                const uint4 *nx = blk + 4 * (b + 1 < blocks ? b + 1 : b);
                const uint4 q0 = nx[0], q1 = nx[1], q2 = nx[2], q3 = nx[3];
                md5::block(state, m);
                const uint32_t v[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
                for (int k = 0; k < 16; k++) m[k] = first(v[k]);
            }
        }
        __syncthreads();                                 // tile t + 1 is complete, and tile t's half may be overwritten
    }
    if (tid == 0) {
        uint32_t *out = hash + (size_t)blockIdx.y * kHashStride + kMd5Word + 4 * c;
        out[0] = state[0]; out[1] = state[1]; out[2] = state[2]; out[3] = state[3];
    }
}

void launch_hevc_md5(const HevcPicParams *d_pics, int n, uint32_t *d_hash, hipStream_t st) {
    hipLaunchKernelGGL(k_hevc_md5, dim3(3, n), dim3(256), 0, st, d_pics, d_hash);
}

void launch_hevc_pichash(const HevcPicParams *d_pics, int n, int max_h, uint32_t *d_hash, hipStream_t st) {
    hipMemsetAsync(d_hash, 0, sizeof(uint32_t) * (size_t)n * kHashStride, st);
    if (!upload_pow_tables()) return;                  // (the error stays with the runtime: the caller's hipGetLastError reports it)
    hipLaunchKernelGGL(k_hevc_pichash, dim3(ph::band_count(max_h), n), dim3(256), 0, st, d_pics, d_hash);
}

}  // namespace jmamd
