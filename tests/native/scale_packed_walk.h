// tests/native/scale_packed_walk.h -- k_scale_pack played on the CPU: every tile of a job, 256 lanes per tile, the kernel's own lane routines
// (jmcodec_amd/csrc/scale_packed.h) in the kernel's own order; the end of a loop over the lanes is a barrier, the LDS buffer is heap memory of the
// kernel's size.  Shared by tests/native/scale_packed_check.cpp, rgb_packed_walk.h and tools/out_packed_asan.cpp.  Test infrastructure only.
#pragma once
#include "../../jmcodec_amd/csrc/scale_packed.h"

namespace walk {
using namespace jmamd;

// the four tap tables of a geometry in host memory (upload_scale_tables' counterpart); false: a ratio outside the limits
struct Tables {
    std::vector<int32_t> first[4]; std::vector<int16_t> w[4];
    bool build(int cw, int ch, int tw, int th, ScaleAxis ax[4]) {
        const int S[4] = {cw, ch, cw / 2, ch / 2}, D[4] = {tw, th, tw / 2, th / 2};
        for (int a = 0; a < 4; a++) {
            const int T = build_scale_taps(S[a], D[a], first[a], w[a]);
            if (T < 0 || T > kScaleMaxTaps) return false;
            ax[a] = ScaleAxis{first[a].data(), w[a].data(), T, S[a]};
        }
        return true;
    }
};

// k_scale_pack over one job; false: a tile hit the row guard (the kernel would leave it unwritten)
inline bool scale_frame(const ScaleJob &jb) {
    std::vector<int16_t> hbuf(scl::kScaleMaxRows * scl::kScaleTileW);
    for (int t = 0; t < scl::tiles(jb.tw, jb.th); t++) {
        scl::PlaneTile pt;
        if (!scl::scale_tile(jb, t, pt)) return false;
        for (int tid = 0; tid < 256; tid++) scl::hpass_lane(pt, tid, hbuf.data());
        for (int tid = 0; tid < 256; tid++) scl::vpass_store_lane(jb, pt, tid, hbuf.data());
    }
    return true;
}

}  // namespace walk
