// tests/native/deint2_packed_check.cpp -- host build of jmcodec_amd/csrc/deint2_packed.h (the strip routine of k_deint2) behind a C ABI, so that
// tests/test_field_rate_host.py can check it against the numpy restatement of the function D without a GPU.  Test infrastructure only.
#include "../../jmcodec_amd/csrc/deint2_packed.h"
using namespace jmamd::dei;
extern "C" {
// one plane: H rows of W bytes (step 1: a luma plane; step 2: an interleaved chroma plane, W = 2 * chroma width), every strip of every chunk as the
// kernel's lanes walk them.  top / bot: the outputs that keep the even / the odd rows; split: each is two planes of W / 2 bytes per row (I420),
// top1 / bot1 the second ones.
void dei2_plane(const uint8_t *src, int pitch, int W, int H, int step, int mode, int threshold, uint8_t *top, uint8_t *top1, uint8_t *bot, uint8_t *bot1,
                int dst_pitch, int split) {
    const PlaneOut o0{top, top1, dst_pitch, split != 0}, o1{bot, bot1, dst_pitch, split != 0};
    for (int k = 0; k < strip2_count(H); k++)
        for (int x = 0; x < W; x += 16) {
            if (step == 1) deint2_strip<1>(src, pitch, W, H, x, k, mode, 4 * threshold * threshold, o0, o1);
            else deint2_strip<2>(src, pitch, W, H, x, k, mode, 4 * threshold * threshold, o0, o1);
        }
}
// one frame, every work item of k_deint2 in turn, with the kernel's own mapping of a job's destinations: dst_first keeps first_parity, dst_second the other
void dei2_frame(const uint8_t *src, int pitch, int chroma_offset, int w, int h, int mode, int first_parity, int threshold, uint8_t *dst_first,
                uint8_t *dst_second, int dst_pitch, int dst_chroma_offset, int out_fmt) {
    for (int i = 0; i < frame2_items(w, h); i++)
        deint2_item(src, first_parity ? dst_second : dst_first, first_parity ? dst_first : dst_second, pitch, chroma_offset, w, h, dst_pitch,
                    dst_chroma_offset, out_fmt, mode, 4 * threshold * threshold, i);
}
int dei2_strip_rows() { return kDeintStrip; }
}
