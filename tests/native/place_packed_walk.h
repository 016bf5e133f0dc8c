// tests/native/place_packed_walk.h -- placed jobs (INTEGRATION.md "Placed output") played on the CPU: k_scale_pack and both k_rgb_pack instantiations
// over a job whose picture fills a rectangle of the target, the kernels' own lane routines in the kernels' own order (out_kernels.hip).  The tap tables
// are those of crop -> rectangle, each vector of exactly its size, so a table index outside [0, rw) / [0, rh) is a heap overflow under
// AddressSanitizer.  Needs clang (_Float16).  Shared by tests/native/place_packed_check.cpp and tools/place_packed_asan.cpp.  Test infrastructure only.
#pragma once
#include "rgb_packed_walk.h"

namespace walk {

// the rectangle and the fill of a job, and its tables; rect w / h == 0: no placement (the tables are crop -> target)
inline bool place(ScaleJob &sj, Tables &tables, int cw, int ch, const int rect[4], int fill, bool need_tables = true) {
    const bool placed = rect[2] != 0 && !(rect[0] == 0 && rect[1] == 0 && rect[2] == sj.tw && rect[3] == sj.th);
    if (placed) { sj.rx = rect[0]; sj.ry = rect[1]; sj.rw = rect[2]; sj.rh = rect[3]; sj.fill = fill; }
    return !need_tables || tables.build(cw, ch, placed ? rect[2] : sj.tw, placed ? rect[3] : sj.th, sj.ax);
}

// k_scale_pack over one placed job: the kernel is the unplaced one's, tile by tile on the target grid
inline bool placed_scale_frame(const ScaleJob &jb) { return scale_frame(jb); }

// k_rgb_pack<false> / <true> over one job, placed or not, as the kernel runs it
inline bool placed_rgb_frame(const RgbJob &jb) {
    const ScaleJob &sj = jb.s;
    std::vector<int16_t> hy(scl::kScaleMaxRows * scl::kRgbTileW), hc(scl::kScaleMaxRows * scl::kRgbTileW);
    std::vector<uint8_t> gcv((scl::kRgbTileH / 2) * scl::kRgbTileW);
    uint8_t (*gc)[scl::kRgbTileW] = reinterpret_cast<uint8_t (*)[scl::kRgbTileW]>(gcv.data());
    for (int t = 0; t < scl::rgb_tiles(sj.tw, sj.th); t++) {
        rgbp::Tile tl;
        if (!rgbp::tile(sj, t, tl)) return false;
        int Y[256][4], U[256][2], V[256][2];                   // the lanes' registers
        for (int tid = 0; tid < 256; tid++) for (int k = 0; k < 4; k++) { Y[tid][k] = 0; U[tid][k >> 1] = V[tid][k >> 1] = 128; }
        if (!jb.identity) {
            scl::PlaneTile ly, lc;
            if (!scl::plane_tile(sj, false, tl.j0, tl.i0, tl.jn, tl.in, ly) || !scl::plane_tile(sj, true, tl.j0 >> 1, tl.i0 >> 1, tl.jn >> 1, tl.in >> 1, lc))
                return false;
            for (int tid = 0; tid < 256; tid++) { scl::hpass_lane(ly, tid, hy.data()); scl::hpass_lane(lc, tid, hc.data()); }
            for (int tid = 0; tid < 256; tid++) { rgbp::vpass_chroma_lane(lc, tid, hc.data(), gc); if ((tid >> 4) < tl.in) rgbp::vpass_luma_lane(ly, tid, hy.data(), Y[tid]); }
            for (int tid = 0; tid < 256; tid++) if ((tid >> 4) < tl.in) rgbp::chroma_lane(tid, gc, U[tid], V[tid]);
        } else {
            for (int tid = 0; tid < 256; tid++) {
                const int r = tid >> 4, q = tid & 15;
                if (r >= tl.in) continue;
                if (!sj.rw) rgbp::fetch_identity(sj, tl.i0 + r, tl.j0 + 4 * q, tl.jn - 4 * q, Y[tid], U[tid], V[tid]);
                else rgbp::fetch_placed(sj, tl.i0 + r, tl.j0 + 4 * q, rgbp::inside_mask(sj, tl.i0 + r, tl.j0 + 4 * q), Y[tid], U[tid], V[tid]);
            }
        }
        for (int tid = 0; tid < 256; tid++) {
            const int r = tid >> 4, q = tid & 15, n = scl::imin(4, tl.jn - 4 * q);
            if (r >= tl.in || n <= 0) continue;
            rgbp::convert_store_masked(jb, Y[tid], U[tid], V[tid], (size_t)(tl.i0 + r) * sj.tw + tl.j0 + 4 * q, n, rgbp::inside_mask(sj, tl.i0 + r, tl.j0 + 4 * q));
        }
    }
    return true;
}

}  // namespace walk
