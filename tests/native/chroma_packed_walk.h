// tests/native/chroma_packed_walk.h -- k_rgb_pack444 played on the CPU, as rgb_packed_walk.h plays k_rgb_pack: the lane routines of
// jmcodec_amd/csrc/chroma_packed.h in the kernel's own order (out_kernels.hip), the end of a loop over the lanes a barrier, the LDS buffers heap memory
// of the kernel's size.  The six tap tables are vectors of exactly their size, so a table index outside its axis is a heap overflow under
// AddressSanitizer.  Needs clang (_Float16).  Shared by tests/native/chroma_packed_check.cpp and tools/chroma_packed_asan.cpp.  Test infrastructure only.
#pragma once
#include "../../jmcodec_amd/csrc/chroma_packed.h"
#include "place_packed_walk.h"

namespace walk {

// the two chroma tables of a geometry in host memory (upload_chroma_tables' counterpart): crop cw x ch -> dw x dh (the target, or the rectangle)
struct ChromaTables {
    std::vector<int32_t> first[2]; std::vector<int16_t> w[2];
    bool build(int cw, int ch, int dw, int dh, int loc, ScaleAxis cax[2]) {
        const int S[2] = {cw / 2, ch / 2}, D[2] = {dw, dh}, q[2] = {chr::siting_qx(loc), chr::siting_qy(loc)};
        for (int a = 0; a < 2; a++) {
            const int T = build_chroma_taps(S[a], D[a], q[a], first[a], w[a]);
            if (T < 0 || T > chr::kChromaMaxTaps) return false;
            cax[a] = ScaleAxis{first[a].data(), w[a].data(), T, S[a]};
        }
        return true;
    }
};

// k_rgb_pack444 over one job (RgbJob::chroma == 1), placed or not; false: a tile hit a row guard
inline bool chroma_rgb_frame(const RgbJob &jb) {
    const ScaleJob &sj = jb.s;
    std::vector<int16_t> hy(scl::kScaleMaxRows * scl::kRgbTileW), hc(2 * chr::kChromaMaxRows * scl::kRgbTileW);
    for (int t = 0; t < scl::rgb_tiles(sj.tw, sj.th); t++) {
        rgbp::Tile tl;
        if (!rgbp::tile(sj, t, tl)) return false;
        scl::PlaneTile ly, lc[2];
        if (!scl::plane_tile(sj, false, tl.j0, tl.i0, tl.jn, tl.in, ly) || !chr::chroma_tiles(jb, ly, lc)) return false;
        for (int tid = 0; tid < 256; tid++) { scl::hpass_lane(ly, tid, hy.data()); chr::hpass_chroma_lane(lc, tid, hc.data()); }
        for (int tid = 0; tid < 256; tid++) {
            const int r = tid >> 4, q = tid & 15, n = scl::imin(4, tl.jn - 4 * q);
            if (r >= tl.in || n <= 0) continue;
            const uint32_t inside = rgbp::inside_mask(sj, tl.i0 + r, tl.j0 + 4 * q);
            int Y[4] = {0, 0, 0, 0}, U[4] = {128, 128, 128, 128}, V[4] = {128, 128, 128, 128};
            rgbp::vpass_luma_lane(ly, tid, hy.data(), Y);
            chr::vpass_chroma_lane(lc, tid, hc.data(), inside, U, V);
            chr::convert_store_444(jb, Y, U, V, (size_t)(tl.i0 + r) * sj.tw + tl.j0 + 4 * q, n, inside);
        }
    }
    return true;
}

}  // namespace walk
