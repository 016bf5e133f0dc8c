// jmcodec_amd/csrc/jpeg_recon.h -- the sample arithmetic of MJPEG decode (codec_type 2), INTEGRATION.md "MJPEG": dequantisation, the two passes of the
// integer IDCT and the chroma rules, as __host__ __device__ functions.  k_jpeg_recon (jpeg_kernels.hip) and the host reconstruction below run the
// same routines, so the CPU checks (tests/native/jpeg_check.cpp, tools/fuzz_jpeg.cpp) exercise the kernel's own arithmetic.  All int32, >> arithmetic.
#pragma once
#include <stdint.h>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JR_HD __host__ __device__ __forceinline__
#define JR_UNROLL _Pragma("unroll")
#else
#define JR_HD inline
#define JR_UNROLL
#endif

namespace jmamd {

// M[k][n] = rint(8192 c_k cos((2n + 1) k pi / 16)), c_0 = 1 / sqrt(8), c_k = 1 / 2.  Sum_k |M[k][n]| <= 21641: with |F| <= 32768 the first sum stays
// below 7.1e8, with |g| <= 65536 the second below 1.42e9 -- both inside int32.
JR_HD int jpeg_m(int k, int n) {
    const int16_t m[64] = {
        2896,  2896,  2896,  2896,  2896,  2896,  2896,  2896,
        4017,  3406,  2276,   799,  -799, -2276, -3406, -4017,
        3784,  1567, -1567, -3784, -3784, -1567,  1567,  3784,
        3406,  -799, -4017, -2276,  2276,  4017,   799, -3406,
        2896, -2896, -2896,  2896,  2896, -2896, -2896,  2896,
        2276, -4017,   799,  3406, -3406,  -799,  4017, -2276,
        1567, -3784,  3784, -1567, -1567,  3784, -3784,  1567,
         799, -2276,  3406, -4017,  4017, -3406,  2276,  -799};
    return m[k * 8 + n];
}

// natural (raster) index v * 8 + u of zig-zag position k
JR_HD int jpeg_zigzag(int k) {
    const uint8_t zz[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return zz[k & 63];
}

JR_HD int jpeg_clip(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }

// F[v][u] = clip(-32768, 32767, level * Q)
JR_HD int jpeg_dequant(int level, int q) { return jpeg_clip(-32768, 32767, level * q); }

// first pass, one column u: g[y] = clip(-65536, 65535, (sum_v M[v][y] F[v] + 256) >> 9)
JR_HD void jpeg_pass1(const int F[8], int g[8]) {
JR_UNROLL
    for (int y = 0; y < 8; y++) {
        int s = 256;
JR_UNROLL
        for (int v = 0; v < 8; v++) s += jpeg_m(v, y) * F[v];
        g[y] = jpeg_clip(-65536, 65535, s >> 9);
    }
}

// second pass, one row y: sample[x] = clip(0, 255, ((sum_u M[u][x] g[u] + 65536) >> 17) + 128)
JR_HD void jpeg_pass2(const int g[8], uint8_t s[8]) {
JR_UNROLL
    for (int x = 0; x < 8; x++) {
        int a = 65536;
JR_UNROLL
        for (int u = 0; u < 8; u++) a += jpeg_m(u, x) * g[u];
        s[x] = (uint8_t)jpeg_clip(0, 255, (a >> 17) + 128);
    }
}

// chroma of a 4:2:2 picture: two rows to one; of a 4:4:4 picture: a 2x2 cell to one
JR_HD int jpeg_avg2(int a, int b) { return (a + b + 1) >> 1; }
JR_HD int jpeg_avg4(int a, int b, int c, int d) { return (a + b + c + d + 2) >> 2; }

// one block: its entries (position | level << 16) and the component's table (zig-zag order) -> 64 samples in raster order
inline void jpeg_block_host(const uint32_t *entries, int count, const uint8_t q[64], uint8_t out[64]) {
    int F[64] = {0}, g[64];
    for (int i = 0; i < count; i++) { const int k = (int)(entries[i] & 63); F[jpeg_zigzag(k)] = jpeg_dequant((int16_t)(entries[i] >> 16), q[k]); }
    for (int u = 0; u < 8; u++) { int col[8], o[8]; for (int v = 0; v < 8; v++) col[v] = F[v * 8 + u]; jpeg_pass1(col, o);
        for (int y = 0; y < 8; y++) g[y * 8 + u] = o[y]; }
    for (int y = 0; y < 8; y++) jpeg_pass2(g + y * 8, out + y * 8);
}

// Host reconstruction of a whole picture from its job list: the tight NV12 frame of dw x dh samples (dw, dh even) that the device's surface shows.
// sampling / block counts as in JpegPicParams (jpeg_jobs.h).  Records that point outside the entry list count as empty blocks, as on the device.
inline void jpeg_reconstruct_host(int sampling, int y_bw, int y_bh, int c_bw, int c_bh, const uint32_t *first, const uint8_t *count,
                                  const uint32_t *entries, size_t n_entries, const uint8_t q[3][64], int dw, int dh, std::vector<uint8_t> &nv12) {
    nv12.assign((size_t)dw * dh * 3 / 2, 128);
    auto block = [&](size_t idx, int comp, uint8_t out[64]) {
        int n = count[idx]; if ((size_t)first[idx] + (size_t)n > n_entries) n = 0;
        jpeg_block_host(entries + (n ? first[idx] : 0), n, q[comp], out);
    };
    uint8_t s[64];
    for (int by = 0; by < y_bh; by++) for (int bx = 0; bx < y_bw; bx++) {
        block((size_t)by * y_bw + bx, 0, s);
        for (int y = 0; y < 8; y++) for (int x = 0; x < 8; x++) if (by * 8 + y < dh && bx * 8 + x < dw) nv12[(size_t)(by * 8 + y) * dw + bx * 8 + x] = s[y * 8 + x];
    }
    if (sampling == 0x10) return;
    const size_t nY = (size_t)y_bw * y_bh, nC = (size_t)c_bw * c_bh;
    uint8_t *uv = nv12.data() + (size_t)dw * dh;
    for (int c = 0; c < 2; c++) for (int by = 0; by < c_bh; by++) for (int bx = 0; bx < c_bw; bx++) {
        block(nY + c * nC + (size_t)by * c_bw + bx, 1 + c, s);
        if (sampling == 0x22) { for (int y = 0; y < 8; y++) for (int x = 0; x < 8; x++) if (by * 8 + y < dh / 2 && bx * 8 + x < dw / 2)
            uv[(size_t)(by * 8 + y) * dw + (bx * 8 + x) * 2 + c] = s[y * 8 + x]; }
        else if (sampling == 0x21) { for (int y = 0; y < 4; y++) for (int x = 0; x < 8; x++) if (by * 4 + y < dh / 2 && bx * 8 + x < dw / 2)
            uv[(size_t)(by * 4 + y) * dw + (bx * 8 + x) * 2 + c] = (uint8_t)jpeg_avg2(s[2 * y * 8 + x], s[(2 * y + 1) * 8 + x]); }
        else { for (int y = 0; y < 4; y++) for (int x = 0; x < 4; x++) if (by * 4 + y < dh / 2 && bx * 4 + x < dw / 2)
            uv[(size_t)(by * 4 + y) * dw + (bx * 4 + x) * 2 + c] = (uint8_t)jpeg_avg4(s[2 * y * 8 + 2 * x], s[2 * y * 8 + 2 * x + 1], s[(2 * y + 1) * 8 + 2 * x],
                                                                                         s[(2 * y + 1) * 8 + 2 * x + 1]); }
    }
}

}  // namespace jmamd
