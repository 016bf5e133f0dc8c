// tests/native/mpeg2_field_vlc_check.cpp -- options mpeg2_device_vlc and mpeg2_field_pictures together, on the CPU: the device routine
// (mpeg2_vlc_slice, the code k_mpeg2_vlc runs) walked over every slice of every FRAME picture of a stream (mpeg2_vlc_walk.h) next to the host
// decoder mpeg2_decode_picture, with the splitter's switch on or off.  Field pictures take the host path in the product and are skipped here.
// Built with g++ by tests/test_mpeg2_field_host.py.
#include "mpeg2_vlc_walk.h"

using namespace jmamd;

extern "C" {
// info (16 ints): [0] frame pictures walked, [1] macroblocks that differ from the host's (records without `first`, per-block entry lists), [2]
// pictures with the dual-prime status, [3] dual-prime records of the walk, [4] of the host decoder, [5] pictures the host decoder refused, [6]
// pictures whose error flag differs, [7] clamped macroblocks of the walk, [8] of the host decoder, [9] a bound was broken or the spans did not
// tile, [10] field pictures skipped, [11] pictures the prescan sent to the host path, [12] kinds of damage the walk met (1 << kind).
// Returns 0, or -1 when the splitter refused the stream.
long m2fv_stream(const uint8_t *data, long n, int field_pictures, int *info) {
    Mpeg2Splitter sp; Mpeg2Jobs jobs; Mpeg2VlcWalk w;
    sp.field_pictures = field_pictures != 0;
    for (int i = 0; i < 16; i++) info[i] = 0;
    auto sink = [&](Mpeg2Pic &pic) {
        if (!pic.have_ext) return;
        if (pic.field()) { info[10]++; return; }
        bool refuse = false;
        const std::string e = mpeg2_decode_picture(pic, jobs, &refuse);
        mpeg2_vlc_walk(pic, w);
        if (!w.reject.empty()) { info[11]++; return; }
        info[0]++; info[2] += w.dual_prime; info[5] += refuse; info[9] += !w.bound_ok || !w.tiled; info[12] |= (int)w.kinds;
        for (const Mpeg2Mb &m : w.mbs) info[3] += (m.flags & M2_DUAL) != 0;
        if (refuse || w.dual_prime) return;                      // (the handle fails on both paths: nothing to compare)
        info[4] += jobs.n_dual;
        info[1] += (int)mpeg2_vlc_compare(w, jobs);
        info[6] += w.error() != !e.empty();
        info[7] += w.clamped; info[8] += jobs.clamped;
    };
    sp.feed(data, (size_t)n, sink);
    sp.flush(sink);
    return sp.refused() ? -1 : 0;
}
}
