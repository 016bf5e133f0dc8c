// tests/native/rgb_packed_walk.h -- k_rgb_pack played on the CPU, as scale_packed_walk.h plays k_scale_pack: the lane routines of
// jmcodec_amd/csrc/rgb_packed.h in the kernel's own order, the lanes' registers that live across a barrier in arrays.  Needs clang (_Float16).
// Shared by tests/native/rgb_packed_check.cpp and tools/out_packed_asan.cpp.  Test infrastructure only.
#pragma once
#include "../../jmcodec_amd/csrc/rgb_packed.h"
#include "scale_packed_walk.h"

namespace walk {

// k_rgb_pack<false> / <true> over one job (the instantiation of its kind)
inline bool rgb_frame(const RgbJob &jb) {
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
            for (int tid = 0; tid < 256; tid++)
                if ((tid >> 4) < tl.in) rgbp::fetch_identity(sj, tl.i0 + (tid >> 4), tl.j0 + 4 * (tid & 15), tl.jn - 4 * (tid & 15), Y[tid], U[tid], V[tid]);
        }
        for (int tid = 0; tid < 256; tid++) {
            const int r = tid >> 4, q = tid & 15, n = scl::imin(4, tl.jn - 4 * q);
            if (r >= tl.in || n <= 0) continue;
            rgbp::convert_store(jb, Y[tid], U[tid], V[tid], (size_t)(tl.i0 + r) * sj.tw + tl.j0 + 4 * q, n);
        }
    }
    return true;
}

}  // namespace walk
