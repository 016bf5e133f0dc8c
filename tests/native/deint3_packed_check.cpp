// tests/native/deint3_packed_check.cpp -- host build of jmcodec_amd/csrc/deint3_packed.h (the strip routine of k_deint3) behind a C ABI, so that
// tests/test_deint3_host.py can check it against the numpy restatement of the function D3 without a GPU.  Test infrastructure only.
#include "../../jmcodec_amd/csrc/deint3_packed.h"
using namespace jmamd::dei;
extern "C" {
// one plane: H rows of W bytes (step 1: a luma plane; step 2: an interleaved chroma plane, W = 2 * chroma width) against the plane `prev`, every strip
// of every chunk as the kernel's lanes walk them.  both: top / bot are the outputs that keep the even / the odd rows; else only the one that keeps
// parity p is written (the other may be null).  split: each is two planes of W / 2 bytes per row (I420), top1 / bot1 the second ones.
void dei3_plane(const uint8_t *src, int pitch, const uint8_t *prev, int prev_pitch, int W, int H, int step, int p, int both, int threshold, uint8_t *top,
                uint8_t *top1, uint8_t *bot, uint8_t *bot1, int dst_pitch, int split) {
    PlaneOut o0{top, top1, dst_pitch, split != 0}, o1{bot, bot1, dst_pitch, split != 0};
    if (!both) { if (p) o0 = o1; else o1 = o0; }
    for (int k = 0; k < strip2_count(H); k++)
        for (int x = 0; x < W; x += 16) {
            if (step == 1) deint3_strip<1>(src, pitch, prev, prev_pitch, W, H, x, k, p, both != 0, threshold, o0, o1);
            else deint3_strip<2>(src, pitch, prev, prev_pitch, W, H, x, k, p, both != 0, threshold, o0, o1);
        }
}
// one frame, every work item of k_deint3 in turn: dst keeps `parity`, dst2 (may be null) the other one
void dei3_frame(const uint8_t *src, int pitch, int chroma_offset, const uint8_t *prev, int prev_pitch, int prev_chroma_offset, int w, int h, int parity,
                int threshold, uint8_t *dst, uint8_t *dst2, int dst_pitch, int dst_chroma_offset, int out_fmt) {
    for (int i = 0; i < frame2_items(w, h); i++)
        deint3_item(src, prev, dst, dst2, pitch, chroma_offset, prev_pitch, prev_chroma_offset, w, h, dst_pitch, dst_chroma_offset, out_fmt, parity,
                    threshold, i);
}
int dei3_strip_rows() { return kDeintStrip; }
}
