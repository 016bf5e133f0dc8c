// tests/native/place_packed_check.cpp -- host build of the placed paths of jmcodec_amd/csrc/scale_packed.h and rgb_packed.h behind a C ABI, so that
// tests/test_placed_output_host.py can check whole frames against the numpy restatement of "Placed output" without a GPU.  Built with clang (_Float16).
// Test infrastructure only.
#include "place_packed_walk.h"
using namespace jmamd;
extern "C" {
// one job as k_scale_pack sees it, the picture placed at rect = x, y, w, h of the target (w == 0: no placement); fill = Y << 16 | Cb << 8 | Cr.
// 0, -1: a ratio outside the limits, -2: a tile hit the row guard
int place_scl_frame(const uint8_t *src, int pitch, int chroma_offset, int lone_field, int crop_x, int crop_y, int crop_w, int crop_h, int tw, int th, int out_fmt,
                    const int *rect, int fill, uint8_t *dst) {
    ScaleJob job{src, dst, pitch, chroma_offset, crop_x, crop_y, tw, th, out_fmt, lone_field, {}};
    walk::Tables tables;
    if (!walk::place(job, tables, crop_w, crop_h, rect, fill)) return -1;
    return walk::placed_scale_frame(job) ? 0 : -2;
}
// ... and as k_rgb_pack sees it (the instantiation of the job's kind: identity = the rectangle has the crop's size); fill = R << 16 | G << 8 | B
int place_rgb_frame(const uint8_t *src, int pitch, int chroma_offset, int lone_field, int crop_x, int crop_y, int crop_w, int crop_h, int tw, int th,
                    const int *coefs, int full_range, int dtype, int planar, int bgr, const float *scale, const float *bias, const int *rect, int fill,
                    uint8_t *dst) {
    RgbJob job = {};
    job.s = ScaleJob{src, dst, pitch, chroma_offset, crop_x, crop_y, tw, th, 0, lone_field, {}};
    job.cy = coefs[0]; job.crv = coefs[1]; job.cgu = coefs[2]; job.cgv = coefs[3]; job.cbu = coefs[4]; job.yo = full_range ? 0 : 16;
    job.dtype = dtype; job.planar = planar; job.bgr = bgr; job.fill = fill;
    for (int k = 0; k < 3; k++) { job.k[k] = scale[k] * (1.0f / 16384.0f); job.b[k] = bias[k]; }
    const int rw = rect[2] ? rect[2] : tw, rh = rect[2] ? rect[3] : th;
    job.identity = rw == crop_w && rh == crop_h;
    walk::Tables tables;
    if (!walk::place(job.s, tables, crop_w, crop_h, rect, 0, !job.identity)) return -1;
    return walk::placed_rgb_frame(job) ? 0 : -2;
}
}
