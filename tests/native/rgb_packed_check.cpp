// tests/native/rgb_packed_check.cpp -- host build of jmcodec_amd/csrc/rgb_packed.h (the lane routines of both k_rgb_pack instantiations) behind a C ABI,
// so that tests/test_rgb_output_host.py can check whole frames against the numpy restatement of C(R_G(F)) without a GPU.  Built with clang (_Float16).
// Test infrastructure only.
#include "rgb_packed_walk.h"
using namespace jmamd;
extern "C" {
// one job as k_rgb_pack sees it: a pitch-linear NV12 surface -> the RGB frame at dst.  coefs: cy, crv, cgu, cgv, cbu (jm_amddec_color_coefs); scale / bias
// as in the spec (the job's k is scale / 16384, exact).  0, -1: a ratio outside the limits, -2: a tile hit the row guard
int rgbp_frame(const uint8_t *src, int pitch, int chroma_offset, int lone_field, int crop_x, int crop_y, int crop_w, int crop_h, int tw, int th,
               const int *coefs, int full_range, int dtype, int planar, int bgr, const float *scale, const float *bias, uint8_t *dst) {
    RgbJob job = {};
    job.s = ScaleJob{src, dst, pitch, chroma_offset, crop_x, crop_y, tw, th, 0, lone_field, {}};
    job.identity = tw == crop_w && th == crop_h;
    job.cy = coefs[0]; job.crv = coefs[1]; job.cgu = coefs[2]; job.cgv = coefs[3]; job.cbu = coefs[4]; job.yo = full_range ? 0 : 16;
    job.dtype = dtype; job.planar = planar; job.bgr = bgr;
    for (int k = 0; k < 3; k++) { job.k[k] = scale[k] * (1.0f / 16384.0f); job.b[k] = bias[k]; }
    walk::Tables tables;
    if (!job.identity && !tables.build(crop_w, crop_h, tw, th, job.s.ax)) return -1;
    return walk::rgb_frame(job) ? 0 : -2;
}
}
