// jmcodec_amd/csrc/out_kernels.hip -- gfx950 output kernels of the jm_amd_dec backend: what turns a decoded surface into the frame the caller gets.
//
// The device half of the reference's host repack, jm_nvdec_output_frame (/root/reference/nv_dec/nv_dec.cpp:750-828), and of the options on top of it:
//   k_packout       pitch NV12 surface -> tight NV12 / I420 display frame
//   k_scale_pack    ... cropped and resampled (scale_packed.h);  k_rgb_pack  ... and converted to RGB (rgb_packed.h)
//   k_deint         ... deinterlaced (deint_packed.h);  k_deint2  both fields of a frame in one pass (deint2_packed.h)
//   k_deint3        ... deinterlaced against the previous display frame (deint3_packed.h)
//   k_frame_to_argb, k_frame_to_nv12_pitch   tight frame -> ARGB32 / pitch NV12
// All fully parallel, 8-bit integer pixel work: HBM / LDS bound, no MFMA.  The arithmetic of the resampler, the colour step and the deinterlacer lives in
// the four __host__ __device__ headers, which the host tests run on the CPU; the kernels here are set-up, LDS buffers, barriers and calls.
// Launchers are declared in kernels.h.
#include <hip/hip_runtime.h>
#include "jobs.h"
#include "kernels.h"
#include "kernel_common.h"     // clip1
#include "scale_packed.h"      // the resampler (k_scale_pack, k_rgb_pack) and the lone-field row mapping
#include "rgb_packed.h"        // the colour step (k_rgb_pack)
#include "chroma_packed.h"     // interpolated chroma at the stream's siting (k_rgb_pack444)
#include "deint_packed.h"      // deint_strip (k_deint)
#include "deint2_packed.h"     // deint2_strip (k_deint2)
#include "deint3_packed.h"     // deint3_strip (k_deint3)

namespace jmamd {

// ------------------------------------------------------------------------------------------
// k_packout: restates jm_nvdec_output_frame (nv_dec.cpp:782-820) on the device.
// out_fmt 0: tight NV12; out_fmt 1: Y plane, U plane, V plane ("YV12" in the reference's words, I420 order).
// One thread moves 16 source bytes.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_packout(const PackJob *jobs) {
    const PackJob jb = jobs[blockIdx.y];
    const uint8_t *src = jb.src; uint8_t *dst = jb.dst;
    const int pitch = jb.pitch, chroma_offset = jb.chroma_offset, width = jb.width, height = jb.height, out_fmt = jb.out_fmt;
    int chunks_per_row = (width + 15) >> 4;
    int luma_chunks = chunks_per_row * height;
    int h2 = height >> 1, w2 = width >> 1;
    int total = luma_chunks + chunks_per_row * h2;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        bool chroma = i >= luma_chunks;
        int j = chroma ? i - luma_chunks : i;
        int row = j / chunks_per_row, x = (j % chunks_per_row) * 16;
        const int srow = scl::surface_row(row, jb.lone_field);
        const uint8_t *s = src + (chroma ? chroma_offset : 0) + (size_t)srow * pitch + x;
        int n = width - x < 16 ? width - x : 16;
        if (!chroma || out_fmt == 0) {
            uint8_t *d = dst + (chroma ? (size_t)width * height : 0) + (size_t)row * width + x;
            if (n == 16 && ((((uintptr_t)d) & 15) == 0)) *(uint4 *)d = *(const uint4 *)s;
            else for (int k = 0; k < n; k++) d[k] = s[k];
        } else {
            uint8_t *du = dst + (size_t)width * height + (size_t)row * w2 + (x >> 1);
            uint8_t *dv = du + (size_t)w2 * h2;
            if (n == 16 && ((((uintptr_t)du) & 7) == 0) && ((((uintptr_t)dv) & 7) == 0)) {
                uint4 v = *(const uint4 *)s;
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
                uint32_t u[2], vv[2];
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    uint32_t a = w[2 * k], b = w[2 * k + 1];
                    u[k] = (a & 0xff) | ((a >> 8) & 0xff00) | ((b & 0xff) << 16) | ((b << 8) & 0xff000000u);
                    vv[k] = ((a >> 8) & 0xff) | ((a >> 16) & 0xff00) | ((b << 8) & 0xff0000) | (b & 0xff000000u);
                }
                *(uint2 *)du = make_uint2(u[0], u[1]); *(uint2 *)dv = make_uint2(vv[0], vv[1]);
            } else for (int k = 0; k < n / 2; k++) { du[k] = s[2 * k]; dv[k] = s[2 * k + 1]; }
        }
    }
}
void launch_packout(const PackJob *d_jobs, int n, int max_width, int max_height, hipStream_t st) {
    int chunks = ((max_width + 15) >> 4) * (max_height + (max_height >> 1));
    int blocks = (chunks + 255) / 256;
    // The destination is pinned HOST memory: the kernel is PCIe-bound (~55 GB/s), not CU-bound.  A small grid is enough to
    // keep the link full and leaves the CUs to the decode kernels of the next batch that run concurrently.
    const int total = 160;
    int cap = total / (n > 0 ? n : 1);
    if (cap < 1) cap = 1;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(k_packout, dim3(blocks, n), dim3(256), 0, st, d_jobs);
}

// Tight I420 / NV12 frame -> 32-bit ARGB (bytes B, G, R, A), BT.601 limited range, the conversion the reference left behind
// "#if 0" (nv_dec.h:98-107, nv_dec.cpp:244-265).  One thread per pixel pair.
__global__ __launch_bounds__(256) void k_frame_to_argb(const uint8_t *src, int w, int h, int fmt, uint8_t *dst, int dst_pitch) {
    int x2 = (blockIdx.x * 256 + threadIdx.x) * 2, y = blockIdx.y;
    if (x2 >= w || y >= h) return;
    const uint8_t *Y = src + (size_t)y * w + x2;
    int u, v;
    if (fmt == 0) { const uint8_t *c = src + (size_t)w * h + (size_t)(y >> 1) * w + (x2 & ~1); u = c[0]; v = c[1]; }
    else { int cw = w >> 1; const uint8_t *pu = src + (size_t)w * h + (size_t)(y >> 1) * cw + (x2 >> 1); u = pu[0]; v = pu[(size_t)cw * (h >> 1)]; }
    int d = u - 128, e = v - 128;
    uint32_t *o = (uint32_t *)(dst + (size_t)y * dst_pitch) + x2;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (x2 + k >= w) break;
        int c = 298 * (Y[k] - 16) + 128;
        int r = clip1((c + 409 * e) >> 8), g = clip1((c - 100 * d - 208 * e) >> 8), b = clip1((c + 516 * d) >> 8);
        o[k] = 0xFF000000u | ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b;
    }
}
void launch_frame_to_argb(const uint8_t *d_src, int w, int h, int fmt, uint8_t *d_dst, int dst_pitch, hipStream_t st) {
    hipLaunchKernelGGL(k_frame_to_argb, dim3((w / 2 + 255) / 256, h), dim3(256), 0, st, d_src, w, h, fmt, d_dst, dst_pitch);
}

// SURVEY 8f f4 -- the encoder-side pre-processing of the reference as a HIP kernel: tight I420 (or tight NV12) frame -> pitch-linear NV12
// surface, i.e. the cuMemcpy2D of the luma plane plus the "InterleaveUV" kernel of /root/reference/nv_enc/nv_enc.cpp:1022-1079 (arguments
// U, V, dst chroma, chroma width / height, source strides, dst stride) in one launch, device to device.  It is the inverse of k_packout.
// One thread per 4 output bytes of a row (luma rows first, then the h/2 interleaved chroma rows).
__global__ __launch_bounds__(256) void k_frame_to_nv12_pitch(const uint8_t *src, int w, int h, int fmt, uint8_t *dst, int pitch) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4, row = blockIdx.y;
    if (x >= w) return;
    uint8_t *o = dst + (size_t)row * pitch + x;
    uint8_t v[4];
    if (row < h || fmt == 0) {                                   // luma row, or an already interleaved chroma row: plain copy
        const uint8_t *i = src + (size_t)row * w + x;
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = x + k < w ? i[k] : 0;
    } else {                                                     // chroma row r: bytes 2c, 2c+1 = U[r][c], V[r][c]
        const int cw = w >> 1, r = row - h;
        const uint8_t *pu = src + (size_t)w * h + (size_t)r * cw, *pv = pu + (size_t)cw * (h >> 1);
#pragma unroll
        for (int k = 0; k < 4; k++) { const int c = (x + k) >> 1; v[k] = x + k < w ? (((x + k) & 1) ? pv[c] : pu[c]) : 0; }
    }
    if (x + 4 <= w && !(pitch & 3)) *(uint32_t *)o = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    else for (int k = 0; k < 4 && x + k < w; k++) o[k] = v[k];
}
void launch_frame_to_nv12_pitch(const uint8_t *d_src, int w, int h, int fmt, uint8_t *d_dst, int pitch, hipStream_t st) {
    hipLaunchKernelGGL(k_frame_to_nv12_pitch, dim3(((w + 3) / 4 + 255) / 256, h + h / 2), dim3(256), 0, st, d_src, w, h, fmt, d_dst, pitch);
}

// ------------------------------------------------------------------------------------------
// k_scale_pack: k_packout with a crop rectangle and a resampler (options crop_* / target_*, INTEGRATION.md "Scaled and cropped output").
// One workgroup per output tile of one plane (scale_packed.h), luma tiles first, then chroma tiles: the horizontal pass writes the tile's filtered
// source rows into LDS as int16, the vertical pass writes 4 output bytes per lane.  A placed job (INTEGRATION.md "Placed output") runs the same two
// calls: the tile's share of the picture's rectangle goes through the passes, the rest of the tile is stored as fill by the same lanes.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_scale_pack(const ScaleJob *jobs) {
    __shared__ int16_t hbuf[scl::kScaleMaxRows * scl::kScaleTileW];   // [source row][64 columns]: luma, or 32 chroma columns x (U, V)
    const ScaleJob &jb = jobs[blockIdx.y];
    scl::PlaneTile t;
    if (!scl::scale_tile(jb, blockIdx.x, t)) return;
    if (!t.placed) {                                          // (uniform per workgroup: an unplaced job runs the passes without the placement arithmetic)
        scl::hpass_lane_t<false>(t, threadIdx.x, hbuf);
        __syncthreads();
        scl::vpass_store_lane_t<false>(jb, t, threadIdx.x, hbuf);
    } else {
        scl::hpass_lane_t<true>(t, threadIdx.x, hbuf);
        __syncthreads();
        scl::vpass_store_lane_t<true>(jb, t, threadIdx.x, hbuf);
    }
}

int scale_tiles(int tw, int th) { return scl::tiles(tw, th); }
void launch_scale_pack(const ScaleJob *d_jobs, int n, int max_tiles, hipStream_t st) {
    if (n > 0 && max_tiles > 0) hipLaunchKernelGGL(k_scale_pack, dim3(max_tiles, n), dim3(256), 0, st, d_jobs);
}

// ------------------------------------------------------------------------------------------
// k_rgb_pack: output C(R_G(F)) -- k_scale_pack's crop and resampler followed by the colour conversion C (INTEGRATION.md "RGB output", rgb_packed.h).
// One workgroup per output tile of 64 x 16 pixels.  Two instantiations over the same job table, each for the jobs of its kind: SCALED = false
// (identity jobs: the picture's size is the crop's, placed or not) uses no LDS, so its occupancy is set by registers alone; SCALED = true holds the two
// passes' LDS buffers.  Pixels outside a placed job's rectangle leave as its fill colour through the same sample step and the same stores.
// ------------------------------------------------------------------------------------------
template <bool SCALED>
__global__ __launch_bounds__(256) void k_rgb_pack(const RgbJob *jobs) {
    const RgbJob &jb = jobs[blockIdx.y];
    // (a job of the other instantiation, or of k_rgb_pack444: such a job is never an identity job, so only the resampling instantiation has to ask)
    if (jb.identity == (SCALED ? 1 : 0) || (SCALED && jb.chroma)) return;
    const ScaleJob &sj = jb.s;
    rgbp::Tile t;
    if (!rgbp::tile(sj, blockIdx.x, t)) return;
    const int tid = threadIdx.x, r = tid >> 4, q = tid & 15;  // the lane's row of the tile and its columns 4q .. 4q + 3
    int Y[4] = {0, 0, 0, 0}, U[2] = {128, 128}, V[2] = {128, 128};
    if constexpr (SCALED) {
        __shared__ int16_t hy[scl::kScaleMaxRows * scl::kRgbTileW];    // luma source rows after the horizontal pass
        __shared__ int16_t hc[scl::kScaleMaxRows * scl::kRgbTileW];    // chroma source rows after the horizontal pass: 32 columns x (U, V)
        __shared__ uint8_t gc[scl::kRgbTileH / 2][scl::kRgbTileW];     // the tile's chroma of G: 8 rows x 32 columns x (U, V)
        scl::PlaneTile ly, lc;
        const bool fits = scl::plane_tile(sj, false, t.j0, t.i0, t.jn, t.in, ly);
        if (!scl::plane_tile(sj, true, t.j0 >> 1, t.i0 >> 1, t.jn >> 1, t.in >> 1, lc) || !fits) return;
        scl::hpass_lane(ly, tid, hy);
        scl::hpass_lane(lc, tid, hc);
        __syncthreads();
        rgbp::vpass_chroma_lane(lc, tid, hc, gc);
        if (r < t.in) rgbp::vpass_luma_lane(ly, tid, hy, Y);
        __syncthreads();
        if (r < t.in) rgbp::chroma_lane(tid, gc, U, V);
    } else if (r < t.in) {
        if (!sj.rw) rgbp::fetch_identity(sj, t.i0 + r, t.j0 + 4 * q, t.jn - 4 * q, Y, U, V);                 // (uniform per workgroup)
        else rgbp::fetch_placed(sj, t.i0 + r, t.j0 + 4 * q, rgbp::inside_mask(sj, t.i0 + r, t.j0 + 4 * q), Y, U, V);
    }
    if (r >= t.in) return;
    const int n = min(4, t.jn - 4 * q);
    if (n <= 0) return;
    // (a placed job: the pixels outside the picture's rectangle are the fill colour)
    rgbp::convert_store_masked(jb, Y, U, V, (size_t)(t.i0 + r) * sj.tw + t.j0 + 4 * q, n, rgbp::inside_mask(sj, t.i0 + r, t.j0 + 4 * q));
}

// ------------------------------------------------------------------------------------------
// k_rgb_pack444: output C(G') -- the jobs of the same table with RgbJob::chroma == 1 (option rgb_chroma, INTEGRATION.md "RGB output", chroma_packed.h).
// G' is 4:4:4: the luma of R_G, and each chroma plane of the crop resampled straight to the full target at the stream's chroma siting.  One workgroup
// per output tile of 64 x 16 pixels: the luma rows go through k_rgb_pack's horizontal pass into hy, the chroma rows through the same pass as two half
// tiles of 32 columns x (U, V) into hc (64 columns x (U, V) per source row), then every lane filters its 4 luma samples and its 4 chroma pairs
// vertically and converts.  Every geometry runs the passes (the luma tables of an identity geometry pass samples through exactly).
// LDS: 17,408 B (hy) + 17,408 B (hc) = 34,816 B, four workgroups per CU.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rgb_pack444(const RgbJob *jobs) {
    const RgbJob &jb = jobs[blockIdx.y];
    if (!jb.chroma) return;                                   // (a job of k_rgb_pack)
    const ScaleJob &sj = jb.s;
    rgbp::Tile t;
    if (!rgbp::tile(sj, blockIdx.x, t)) return;
    __shared__ int16_t hy[scl::kScaleMaxRows * scl::kRgbTileW];            // luma source rows after the horizontal pass
    __shared__ int16_t hc[2 * chr::kChromaMaxRows * scl::kRgbTileW];       // chroma source rows after it: two half tiles of 32 columns x (U, V)
    const int tid = threadIdx.x, r = tid >> 4, q = tid & 15;
    scl::PlaneTile ly, lc[2];
    const bool fits = scl::plane_tile(sj, false, t.j0, t.i0, t.jn, t.in, ly);
    if (!fits || !chr::chroma_tiles(jb, ly, lc)) return;      // (uniform per workgroup)
    scl::hpass_lane(ly, tid, hy);
    chr::hpass_chroma_lane(lc, tid, hc);
    __syncthreads();
    const int n = min(4, t.jn - 4 * q);
    if (r >= t.in || n <= 0) return;
    const uint32_t inside = rgbp::inside_mask(sj, t.i0 + r, t.j0 + 4 * q);
    int Y[4] = {0, 0, 0, 0}, U[4] = {128, 128, 128, 128}, V[4] = {128, 128, 128, 128};
    rgbp::vpass_luma_lane(ly, tid, hy, Y);
    chr::vpass_chroma_lane(lc, tid, hc, inside, U, V);
    chr::convert_store_444(jb, Y, U, V, (size_t)(t.i0 + r) * sj.tw + t.j0 + 4 * q, n, inside);
}

int rgb_tiles(int tw, int th) { return scl::rgb_tiles(tw, th); }
void launch_rgb_pack(const RgbJob *d_jobs, int n, int identity_tiles, int scaled_tiles, int chroma_tiles, hipStream_t st) {
    if (n > 0 && identity_tiles > 0) hipLaunchKernelGGL(k_rgb_pack<false>, dim3(identity_tiles, n), dim3(256), 0, st, d_jobs);
    if (n > 0 && scaled_tiles > 0) hipLaunchKernelGGL(k_rgb_pack<true>, dim3(scaled_tiles, n), dim3(256), 0, st, d_jobs);
    if (n > 0 && chroma_tiles > 0) hipLaunchKernelGGL(k_rgb_pack444, dim3(chroma_tiles, n), dim3(256), 0, st, d_jobs);
}

// ------------------------------------------------------------------------------------------
// k_deint: the deinterlacer D (option deinterlace, INTEGRATION.md "Deinterlaced output") -- k_packout with a vertical stencil.  A pure streaming kernel:
// a lane owns a 16-byte column chunk of one plane and walks a strip of 8 rows with a window of 9 in registers (deint_packed.h: deint_strip), so consecutive lanes read and write
// consecutive 16 bytes of the same rows.  All loads of a strip are issued before the first store; no LDS.  Work items: the luma strips row-major
// (chunk fastest), then the strips of the interleaved chroma plane.  The job's mode and parity are uniform per workgroup (blockIdx.y = job).
// ------------------------------------------------------------------------------------------
// one job's items first, first + stride, ... (the lane's share of the grid: the kernels work these out themselves, where the compiler knows the workgroup's size)
__device__ __forceinline__ void deint_job(const DeintJob &jb, int first, int stride) {
    const dei::gbyte *src = (const dei::gbyte *)jb.src; dei::gbyte *dst = (dei::gbyte *)jb.dst;
    const int total = dei::frame_items(jb.width, jb.height);
    for (int i = first; i < total; i += stride)
        dei::deint_item(src, dst, jb.pitch, jb.chroma_offset, jb.width, jb.height, jb.dst_pitch, jb.dst_chroma_offset, jb.out_fmt, jb.mode, jb.parity, jb.thr, i);
}
__global__ __launch_bounds__(256) void k_deint(const DeintJob *jobs) {
    const DeintJob jb = jobs[blockIdx.y];
    deint_job(jb, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
int deint_items(int w, int h) { return dei::frame_items(w, h); }
void launch_deint(const DeintJob *d_jobs, int n, int max_items, hipStream_t st) {
    if (n > 0 && max_items > 0) hipLaunchKernelGGL(k_deint, dim3((max_items + 255) / 256, n), dim3(256), 0, st, d_jobs);
}

// ------------------------------------------------------------------------------------------
// k_deint2: field-rate deinterlacing (option deinterlace_rate, deint2_packed.h).  A job with a second destination puts out D with its parity kept (dst)
// AND D with the other parity kept (dst2) from one walk over the surface: a lane owns a 16-byte column chunk and 8 output rows, loads its 10 source rows
// once and stores 16.  A job without a second destination is k_deint's work, item by item (the branch is uniform per workgroup), so one launch serves a
// side that mixes both; a side without pairs is launched as k_deint.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void deint2_job(const DeintJob &jb, int first, int stride) {
    if (!jb.dst2) { deint_job(jb, first, stride); return; }
    const dei::gbyte *src = (const dei::gbyte *)jb.src; dei::gbyte *dst = (dei::gbyte *)jb.dst, *dst2 = (dei::gbyte *)jb.dst2;
    const int total = dei::frame2_items(jb.width, jb.height);
    for (int i = first; i < total; i += stride)
        dei::deint2_item(src, jb.parity ? dst2 : dst, jb.parity ? dst : dst2, jb.pitch, jb.chroma_offset, jb.width, jb.height, jb.dst_pitch, jb.dst_chroma_offset,
                         jb.out_fmt, jb.mode, jb.thr, i);
}
__global__ __launch_bounds__(256) void k_deint2(const DeintJob *jobs) {
    const DeintJob jb = jobs[blockIdx.y];
    deint2_job(jb, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
int deint2_items(int w, int h) { return dei::frame2_items(w, h); }
void launch_deint2(const DeintJob *d_jobs, int n, int max_items, hipStream_t st) {
    if (n > 0 && max_items > 0) hipLaunchKernelGGL(k_deint2, dim3((max_items + 255) / 256, n), dim3(256), 0, st, d_jobs);
}

// ------------------------------------------------------------------------------------------
// k_deint3: motion-adaptive deinterlacing (option deinterlace_temporal, deint3_packed.h).  A job with a previous frame puts out D3: a lane owns a 16-byte
// column chunk and 8 rows, loads its 10 rows of the frame and of the previous frame once, keeps the frame's rows and ONE mask register per row, and
// stores 8 rows (or 16: a field-rate pair, both parities from the same masks).  A job without a previous frame is k_deint2's work, item by item (the
// branch is uniform per workgroup), so one launch serves a side that mixes them; a side without such a job is launched as before.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_deint3(const DeintJob *jobs) {
    const DeintJob jb = jobs[blockIdx.y];
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if (!jb.prev) { deint2_job(jb, first, stride); return; }
    const int total = dei::frame2_items(jb.width, jb.height);
    for (int i = first; i < total; i += stride)
        dei::deint3_item((const dei::gbyte *)jb.src, (const dei::gbyte *)jb.prev, (dei::gbyte *)jb.dst, (dei::gbyte *)jb.dst2, jb.pitch, jb.chroma_offset,
                         jb.prev_pitch, jb.prev_chroma_offset, jb.width, jb.height, jb.dst_pitch, jb.dst_chroma_offset, jb.out_fmt, jb.parity, jb.t, i);
}
void launch_deint3(const DeintJob *d_jobs, int n, int max_items, hipStream_t st) {
    if (n > 0 && max_items > 0) hipLaunchKernelGGL(k_deint3, dim3((max_items + 255) / 256, n), dim3(256), 0, st, d_jobs);
}

}  // namespace jmamd
