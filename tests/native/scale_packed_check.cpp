// tests/native/scale_packed_check.cpp -- host build of jmcodec_amd/csrc/scale_packed.h (the lane routines of k_scale_pack) behind a C ABI, so that
// tests/test_scaled_output_host.py can check whole frames against the numpy restatement of R_G without a GPU.  Test infrastructure only.
#include "scale_packed_walk.h"
using namespace jmamd;
extern "C" {
// one job as k_scale_pack sees it: a pitch-linear NV12 surface -> the cropped, resampled tight frame (out_fmt 0 NV12, 1 I420) at dst; the tap tables
// are the library's (build_scale_taps).  0, -1: a ratio outside the limits, -2: a tile hit the row guard
int scl_frame(const uint8_t *src, int pitch, int chroma_offset, int lone_field, int crop_x, int crop_y, int crop_w, int crop_h, int tw, int th, int out_fmt,
              uint8_t *dst) {
    ScaleJob job{src, dst, pitch, chroma_offset, crop_x, crop_y, tw, th, out_fmt, lone_field, {}};
    walk::Tables tables;
    if (!tables.build(crop_w, crop_h, tw, th, job.ax)) return -1;
    return walk::scale_frame(job) ? 0 : -2;
}
}
