// jmcodec_amd/csrc/pichash.hip -- k_hevc_pichash: the CRC and the checksum of the decoded picture hash SEI (H.265 D.3.19) of every picture of a batch
// that asks for them, from the finished surface (INTEGRATION.md "Picture hash"; the arithmetic is pichash_packed.h, which the host walks too).
//
// grid (bands, pictures): a workgroup reads kBandRows luma rows and the chroma rows below them ONCE, 16 bytes per lane and load, and computes both
// hashes of all three components from that read.  Both hashes are sums -- mod 2^32, and over GF(2) once every lane has moved its piece of the CRC to
// its place in the picture (pichash_packed.h) -- so a workgroup reduces its lanes (ds_bpermute inside a wave, an LDS array across the four waves) and
// adds ONE value per result word with a device-scope atomicAdd / atomicXor.  Integer add and xor do not depend on the order of arrival: the words are
// the same in every run, without a slab of partial results and a second pass.  The caller clears the words in front of the launch.
// There is no reference counterpart: the reference's decoder never looks at SEI (/root/reference/nv_dec/nv_dec.cpp:368-403 hands the bytes to cuvid).
#include <hip/hip_runtime.h>
#include <mutex>
#include "hevc_kernels.h"
#include "pichash_packed.h"

namespace jmamd {

__device__ uint16_t g_pichash_pow[ph::kPowLo + ph::kPowHi];      // x^i, i < 256, then x^(256 i), i < 128 (mod P)

__global__ __launch_bounds__(256) void k_hevc_pichash(const HevcPicParams *pics, uint32_t *hash) {
    const HevcPicParams &pp = pics[blockIdx.y];
    if (!pp.hash_mode) return;
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

void launch_hevc_pichash(const HevcPicParams *d_pics, int n, int max_h, uint32_t *d_hash, hipStream_t st) {
    hipMemsetAsync(d_hash, 0, sizeof(uint32_t) * (size_t)n * kHashStride, st);
    if (!upload_pow_tables()) return;                  // (the error stays with the runtime: the caller's hipGetLastError reports it)
    hipLaunchKernelGGL(k_hevc_pichash, dim3(ph::band_count(max_h), n), dim3(256), 0, st, d_pics, d_hash);
}

}  // namespace jmamd
