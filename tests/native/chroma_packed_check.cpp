// tests/native/chroma_packed_check.cpp -- host build of jmcodec_amd/csrc/chroma_packed.h (the lane routines of k_rgb_pack444) behind a C ABI, so that
// tests/test_rgb_chroma_host.py can check whole frames against the numpy restatement of C(G') without a GPU.  Built with clang (_Float16).
// Test infrastructure only.
#include "chroma_packed_walk.h"
using namespace jmamd;
extern "C" {
// one job as k_rgb_pack444 sees it: a pitch-linear NV12 surface -> the RGB frame at dst, chroma interpolated at chroma_sample_loc_type loc; the picture
// placed at rect = x, y, w, h of the target (w == 0: no placement), fill = R << 16 | G << 8 | B.  coefs, scale, bias as rgbp_frame's.
// 0, -1: a ratio outside the limits, -2: a tile hit a row guard
int chroma_rgb_frame(const uint8_t *src, int pitch, int chroma_offset, int lone_field, int crop_x, int crop_y, int crop_w, int crop_h, int tw, int th,
                     const int *coefs, int full_range, int dtype, int planar, int bgr, const float *scale, const float *bias, const int *rect, int fill, int loc,
                     uint8_t *dst) {
    RgbJob job = {};
    job.s = ScaleJob{src, dst, pitch, chroma_offset, crop_x, crop_y, tw, th, 0, lone_field, {}};
    job.cy = coefs[0]; job.crv = coefs[1]; job.cgu = coefs[2]; job.cgv = coefs[3]; job.cbu = coefs[4]; job.yo = full_range ? 0 : 16;
    job.dtype = dtype; job.planar = planar; job.bgr = bgr; job.fill = fill;
    for (int k = 0; k < 3; k++) { job.k[k] = scale[k] * (1.0f / 16384.0f); job.b[k] = bias[k]; }
    job.identity = 0; job.chroma = 1;
    walk::Tables tables; walk::ChromaTables ctables;
    if (!walk::place(job.s, tables, crop_w, crop_h, rect, 0)) return -1;
    if (!ctables.build(crop_w, crop_h, job.s.rw ? job.s.rw : tw, job.s.rw ? job.s.rh : th, loc, job.cax)) return -1;
    return walk::chroma_rgb_frame(job) ? 0 : -2;
}
}
