// jmcodec_amd/csrc/rgb_packed.h -- the colour step C of INTEGRATION.md "RGB output", once (k_rgb_pack, out_kernels.hip).
//
// k_rgb_pack puts out C(R_G(F)): one workgroup of 256 lanes per output tile of 64 x 16 pixels, lane tid owns row tid / 16 of the tile and its columns
// 4 q .. 4 q + 3, q = tid & 15.  C needs luma AND chroma of the same pixels, so a scaled job resamples both in one workgroup: the tile's luma (64 x 16)
// and its chroma (32 x 8, both channels) go through the resampler's horizontal pass (scale_packed.h) into two row buffers, the vertical chroma results
// into a third (gc), then every lane filters 4 luma samples of its row -- the passes are k_scale_pack's own functions, so G is bit-identical.  An
// identity job (picture size == crop size) reads the surface directly, no tap tables.  Then every lane converts its 4 pixels -- 14-bit fixed-point
// accumulators, then the sample type of the job -- and stores 3 x 4 samples.
// A placed job (ScaleJob::rw != 0): pixels outside the picture's rectangle are the job's fill colour, selected per pixel in front of the sample step
// (inside_mask, convert_store_masked); pure padding is an identity job (fetch_placed).
// __host__ __device__ like scale_packed.h: tests/test_rgb_output_host.py walks whole frames through these routines on the CPU
// (tests/native/rgb_packed_check.cpp, built with clang: _Float16) against the numpy restatement of C(R_G(F)).
#pragma once
#include "scale_packed.h"

namespace jmamd {
namespace rgbp {

using scl::kRgbTileW; using scl::kRgbTileH;

JM_HD uint32_t f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
JM_HD uint32_t rgb_u8(int a) { const int v = (a + 8192) >> 14; return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
JM_HD float rgb_f32(int a, float k, float b) {
#pragma clang fp contract(off)
    const int c = a < 0 ? 0 : (a > 255 * 16384 ? 255 * 16384 : a);        // exact in fp32 (< 2^24)
    const float m = (float)c * k;                                           // two roundings, never an FMA: numpy float32 restates them
    return m + b;
}
JM_HD uint32_t f32_to_bf16(float f) {                                      // round to nearest even
    const uint32_t u = f32_bits(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;        // NaN stays a (quiet) NaN
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
JM_HD uint32_t f32_to_f16(float f) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f); }

// W dwords to an address aligned to 4 W bytes: one store
template <int W> JM_HD void store_words(uint8_t *d, const uint32_t *w) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t vec __attribute__((ext_vector_type(W)));
    vec v;
    for (int k = 0; k < W; k++) v[k] = w[k];
    *(vec *)d = v;
#else
    memcpy(d, w, 4 * W);
#endif
}
// 4 consecutive samples of sz bytes (their bit patterns in s[]), n of them valid: one vector store when all are and the address allows it
JM_HD void store4(uint8_t *d, int sz, const uint32_t s[4], int n) {
    if (n <= 0) return;
    const uintptr_t a = (uintptr_t)d;
    if (sz == 1) {
        const uint32_t w[1] = {s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24)};
        if (n >= 4 && !(a & 3)) store_words<1>(d, w);
        else for (int k = 0; k < 4; k++) { if (k < n) d[k] = (uint8_t)s[k]; }
    } else if (sz == 2) {
        const uint32_t w[2] = {s[0] | (s[1] << 16), s[2] | (s[3] << 16)};
        if (n >= 4 && !(a & 7)) store_words<2>(d, w);
        else for (int k = 0; k < 4; k++) { if (k < n) scl::store_u16(d + 2 * k, (uint16_t)s[k]); }
    } else {
        if (n >= 4 && !(a & 15)) store_words<4>(d, s);
        else for (int k = 0; k < 4; k++) { if (k < n) scl::store_u32(d + 4 * k, s[k]); }
    }
}

// tile t of k_rgb_pack's grid: pixels j0 .. j0 + jn - 1, rows i0 .. i0 + in - 1 (jn, in even: tw, th are); false: no such tile of this job
struct Tile { int j0, i0, jn, in; };
JM_HD bool tile(const ScaleJob &sj, int t, Tile &o) {
    const int tw = sj.tw, th = sj.th, ntx = (tw + kRgbTileW - 1) / kRgbTileW;
    if (t >= ntx * ((th + kRgbTileH - 1) / kRgbTileH)) return false;
    o.j0 = (t % ntx) * kRgbTileW; o.i0 = (t / ntx) * kRgbTileH;
    o.jn = scl::imin(kRgbTileW, tw - o.j0); o.in = scl::imin(kRgbTileH, th - o.i0);
    return true;
}

// Scaled job, after the horizontal passes: the vertical chroma pass of lane tid -- its share of the tile's 8 x 64 chroma values of G (c: the chroma tile)
JM_HD void vpass_chroma_lane(const scl::PlaneTile &c, int tid, const int16_t *hc, uint8_t (*gc)[kRgbTileW]) {
    for (int e = tid; e < (kRgbTileH / 2) * kRgbTileW; e += 256) {
        const int rr = e / kRgbTileW, col = e % kRgbTileW;
        const int i = c.i0 + rr, j = c.j0 + (col >> 1);          // (the tile's share of the picture: the whole tile unless the job is placed)
        if (i >= c.ia && i < c.ib && j >= c.ja && j < c.jb) { int v; scl::vpass<1>(c, c.i0 + rr, hc, &col, &v); gc[rr][col] = (uint8_t)v; }
    }
}
// ... and the vertical luma pass: the 4 samples of lane tid (y: the luma tile; the lane's row must be one of the tile's)
JM_HD void vpass_luma_lane(const scl::PlaneTile &y, int tid, const int16_t *hy, int Y[4]) {
    const int r = tid >> 4, q = tid & 15;
    int col[4] = {4 * q, 4 * q + 1, 4 * q + 2, 4 * q + 3};
    if (y.placed) {          // a row outside the picture: nothing; columns outside it are filtered as the nearest inside one (and masked by the caller)
        if (y.i0 + r < y.ia || y.i0 + r >= y.ib || y.ja >= y.jb) return;
        JM_SCL_UNROLL
        for (int e = 0; e < 4; e++) col[e] = scl::imin(scl::imax(col[e], y.ja - y.j0), y.jb - 1 - y.j0);
    }
    scl::vpass<4>(y, y.i0 + r, hy, col, Y);
}
// ... and the lane's chroma of G
JM_HD void chroma_lane(int tid, const uint8_t (*gc)[kRgbTileW], int U[2], int V[2]) {
    const int r = tid >> 4, q = tid & 15;
    JM_SCL_UNROLL
    for (int k = 0; k < 2; k++) { U[k] = gc[r >> 1][2 * (2 * q + k)]; V[k] = gc[r >> 1][2 * (2 * q + k) + 1]; }
}

// Identity geometry: row i of the output, n valid pixels from column x on (n may exceed 4; <= 0: none).  Y = F_Y[crop_y + i][crop_x + x ..], chroma of
// F row (crop_y / 2 + i / 2), byte pairs from crop_x + x on (x is even; k_packout's row mapping)
JM_HD void fetch_identity(const ScaleJob &sj, int i, int x, int n, int Y[4], int U[2], int V[2]) {
    if (n <= 0) return;
    const uint8_t *py = sj.src + (size_t)scl::surface_row(sj.crop_y + i, sj.lone_field) * sj.pitch + sj.crop_x + x;
    const uint8_t *pc = sj.src + sj.chroma_offset + (size_t)scl::surface_row((sj.crop_y >> 1) + (i >> 1), sj.lone_field) * sj.pitch + sj.crop_x + x;
    JM_SCL_UNROLL
    for (int e = 0; e < 4; e++) if (e < n) Y[e] = py[e];
    JM_SCL_UNROLL
    for (int k = 0; k < 2; k++) if (2 * k < n) { U[k] = pc[2 * k]; V[k] = pc[2 * k + 1]; }
}

// Placed jobs: which of the 4 pixels from column x on of output row i lie inside the picture's rectangle (bit e: pixel x + e; x and the rectangle are
// even, so the bits come in pairs).  An unplaced job: all of them.
JM_HD uint32_t inside_mask(const ScaleJob &sj, int i, int x) {
    if (!sj.rw) return 15;
    if (i < sj.ry || i >= sj.ry + sj.rh) return 0;
    return (x >= sj.rx && x < sj.rx + sj.rw ? 3u : 0u) | (x + 2 >= sj.rx && x + 2 < sj.rx + sj.rw ? 12u : 0u);
}
// Identity geometry of a placed job (pure padding): fetch_identity for the pixel pairs of `inside`, from the picture's own row and column
JM_HD void fetch_placed(const ScaleJob &sj, int i, int x, uint32_t inside, int Y[4], int U[2], int V[2]) {
    if (!inside) return;
    const int pi = i - sj.ry, px = sj.crop_x + x - sj.rx;          // (px + 2 k >= crop_x for the pairs of `inside`)
    const uint8_t *py = sj.src + (size_t)scl::surface_row(sj.crop_y + pi, sj.lone_field) * sj.pitch;
    const uint8_t *pc = sj.src + sj.chroma_offset + (size_t)scl::surface_row((sj.crop_y >> 1) + (pi >> 1), sj.lone_field) * sj.pitch;
    JM_SCL_UNROLL
    for (int k = 0; k < 2; k++) if ((inside >> (2 * k)) & 1) {
        Y[2 * k] = py[px + 2 * k]; Y[2 * k + 1] = py[px + 2 * k + 1]; U[k] = pc[px + 2 * k]; V[k] = pc[px + 2 * k + 1]; }
}

// C of the lane's 4 pixels (n of them valid, 1 <= n <= 4), pixel index px = row * tw + column of the first: planar or interleaved stores.  A pixel
// whose bit of `inside` is clear is the job's fill colour: its accumulators are fill << 14, through the same sample step.
JM_HD void convert_store_masked(const RgbJob &jb, const int Y[4], const int U[2], const int V[2], size_t px, int n, uint32_t inside) {
    const ScaleJob &sj = jb.s;
    uint32_t s[3][4];
    const int fR = ((jb.fill >> 16) & 255) << 14, fG = ((jb.fill >> 8) & 255) << 14, fB = (jb.fill & 255) << 14;
    const int fa[3] = {jb.bgr ? fB : fR, fG, jb.bgr ? fR : fB};
    JM_SCL_UNROLL
    for (int e = 0; e < 4; e++) {
        const int yv = jb.cy * (Y[e] - jb.yo), d = U[e >> 1] - 128, f = V[e >> 1] - 128;
        const int aR = yv + jb.crv * f, aG = yv - jb.cgu * d - jb.cgv * f, aB = yv + jb.cbu * d;
        const bool in = (inside >> e) & 1;
        const int a[3] = {in ? (jb.bgr ? aB : aR) : fa[0], in ? aG : fa[1], in ? (jb.bgr ? aR : aB) : fa[2]};          // storage positions
        JM_SCL_UNROLL
        for (int c = 0; c < 3; c++) {
            if (jb.dtype == RGB_U8) s[c][e] = rgb_u8(a[c]);
            else {
                const float v = rgb_f32(a[c], jb.k[c], jb.b[c]);
                s[c][e] = jb.dtype == RGB_F32 ? f32_bits(v) : jb.dtype == RGB_F16 ? f32_to_f16(v) : f32_to_bf16(v);
            }
        }
    }
    const int sz = jb.dtype == RGB_U8 ? 1 : (jb.dtype == RGB_F32 ? 4 : 2);
    if (jb.planar) {
        const size_t P = (size_t)sj.tw * sj.th;
        JM_SCL_UNROLL
        for (int c = 0; c < 3; c++) store4(sj.dst + (c * P + px) * sz, sz, s[c], n);
    } else {
        uint32_t v[12];
        JM_SCL_UNROLL
        for (int e = 0; e < 4; e++) for (int c = 0; c < 3; c++) v[3 * e + c] = s[c][e];
        uint8_t *d = sj.dst + 3 * px * sz;
        JM_SCL_UNROLL
        for (int g = 0; g < 3; g++) store4(d + 4 * g * sz, sz, v + 4 * g, 3 * n - 4 * g);
    }
}
JM_HD void convert_store(const RgbJob &jb, const int Y[4], const int U[2], const int V[2], size_t px, int n) { convert_store_masked(jb, Y, U, V, px, n, 15); }

}  // namespace rgbp
}  // namespace jmamd
