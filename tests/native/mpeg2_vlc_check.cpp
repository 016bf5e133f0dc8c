// tests/native/mpeg2_vlc_check.cpp -- option mpeg2_device_vlc on the CPU: the prescan (mpeg2_slice_scan) and the device routine (mpeg2_vlc_slice, the
// code k_mpeg2_vlc runs) walked over every slice of every picture of a stream (mpeg2_vlc_walk.h), next to the host decoder mpeg2_decode_picture.
// Built with g++ by tests/test_mpeg2_vlc_host.py.
#include "mpeg2_vlc_walk.h"

using namespace jmamd;
static std::string g_err;

extern "C" {
const char *m2v_error() { return g_err.c_str(); }
// Every picture of the stream through both paths.  info (32 ints):
//  [0] pictures, [1] of which the prescan accepted, [2] of which it sent to the host path, [3] macroblocks that differ (records without `first`, per-block
//  entry lists), [4] pictures whose error flag differs, [5] clamped macroblocks of the walk, [6] of the host decoder, [7] damaged slices, [8] a bound
//  was broken (iterations, capacity, entry ranges), [9] the spans did not tile a picture, [10] pictures with the dual-prime status, [11] slices,
//  [12] pictures with the holes status, [13] pictures the walk calls damaged, [14] an undamaged slice filled its capacity exactly, [15] slices that
//  start inside a macroblock row, [16] kinds of damage met (1 << kind), [17] pictures the host decoder refused (dual prime), [18] pictures the host
//  decoder calls damaged, [19] the largest first macroblock_address_increment gap between two slices' first addresses on one row (escape test),
//  [20] the largest number of slices in one picture.
// Returns 0, or -1 when the splitter refused the stream.
long m2v_stream(const uint8_t *data, long n, int *info) {
    Mpeg2Splitter sp; Mpeg2Jobs jobs; Mpeg2VlcWalk w;
    for (int i = 0; i < 32; i++) info[i] = 0;
    g_err.clear();
    auto sink = [&](Mpeg2Pic &pic) {
        if (!pic.have_ext) return;
        info[0]++;
        bool refuse = false;
        const std::string e = mpeg2_decode_picture(pic, jobs, &refuse);
        mpeg2_vlc_walk(pic, w);
        if (!e.empty()) g_err = e;
        info[17] += refuse; info[18] += !e.empty() && !refuse;
        if (!w.reject.empty()) { info[2]++; if (g_err.empty()) g_err = w.reject; return; }
        info[1]++;
        info[7] += w.damaged; info[8] += !w.bound_ok; info[9] += !w.tiled; info[10] += w.dual_prime; info[11] += (int)w.slices.size();
        info[12] += w.holes; info[13] += w.error(); info[14] |= w.cap_reached; info[16] |= (int)w.kinds;
        if ((int)w.slices.size() > info[20]) info[20] = (int)w.slices.size();
        const uint32_t mb_w = (uint32_t)pic.seq.mb_w();
        for (size_t i = 1; i < w.slices.size(); i++) {
            info[15] += w.slices[i].lo % mb_w != 0;
            if (w.slices[i].row == w.slices[i - 1].row && (int)(w.slices[i].lo - w.slices[i - 1].lo) > info[19]) info[19] = (int)(w.slices[i].lo - w.slices[i - 1].lo);
        }
        if (refuse || w.dual_prime) return;                      // (the handle fails on both paths: nothing to compare)
        info[3] += (int)mpeg2_vlc_compare(w, jobs);
        info[4] += w.error() != !e.empty();
        info[5] += w.clamped; info[6] += jobs.clamped;
    };
    sp.feed(data, (size_t)n, sink);
    sp.flush(sink);
    if (sp.refused()) { g_err = sp.error(); return -1; }
    return 0;
}
int m2v_guard() { return kMpeg2SliceGuard; }
unsigned m2v_capacity(unsigned n_bytes, unsigned n_mbs) { return mpeg2_vlc_capacity(n_bytes, n_mbs); }
unsigned m2v_padded(unsigned n_bytes) { return mpeg2_vlc_padded(n_bytes); }
int m2v_table_bytes() { return (int)sizeof(Mpeg2VlcTables); }
const char *m2v_damage_text(int kind) { return mpeg2_vlc_damage_text(kind); }
// the slice table of the stream's LAST picture the prescan accepted: 8 words per slice; returns the number of slices (at most cap)
long m2v_slices(const uint8_t *data, long n, uint32_t *out, long cap) {
    Mpeg2Splitter sp; Mpeg2SliceScan sc; long got = -1;
    auto sink = [&](Mpeg2Pic &pic) {
        if (!pic.have_ext || !mpeg2_slice_scan(pic, sc).empty()) return;
        got = (long)sc.slices.size() < cap ? (long)sc.slices.size() : cap;
        memcpy(out, sc.slices.data(), (size_t)got * sizeof(Mpeg2Slice));
    };
    sp.feed(data, (size_t)n, sink);
    sp.flush(sink);
    return got;
}
}
