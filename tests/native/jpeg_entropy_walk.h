// tests/native/jpeg_entropy_walk.h -- plays k_jpeg_entropy on the CPU: the segmenter (jpeg_segment_scan) and then jpeg_entropy_segment, the
// kernel's own routine, once per segment as the kernel's lanes run it.  Every buffer the device would hold is a heap block of exactly the stated
// size -- tables, segment table, clean bytes with their guard, first / count, entries of exactly the capacity -- so that under AddressSanitizer
// (tools/jpeg_entropy_asan.cpp) a read or write one element outside any of them is caught.  Shared by tests/native/jpeg_entropy_check.cpp.
#pragma once
#include "../../jmcodec_amd/csrc/jpeg_syntax.h"
#include "../../jmcodec_amd/csrc/jpeg_entropy.h"
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace jmamd {

struct JpegEntropyWalk {
    std::vector<JpegSegment> segs; std::vector<uint8_t> clean;     // what the segmenter made (copies, for the caller to look at)
    std::vector<uint32_t> first; std::vector<uint8_t> count; std::vector<uint32_t> entries;      // what the device routine wrote
    std::vector<int> seg_damage; std::vector<uint32_t> seg_used;   // per segment: kind of damage (0: none), entries it wrote
    std::string seg_error;                                         // the segmenter's complaint ("" = none)
    int damaged = 0; bool bound_ok = true, cap_reached = false, covered = true;
};

// exact-size heap copy (malloc: nothing behind the last byte belongs to the block)
template <class T> static T *exact_copy(const T *src, size_t n) {
    T *p = (T *)malloc(n ? n * sizeof(T) : 1);
    if (n) memcpy(p, src, n * sizeof(T));
    return p;
}

inline void jpeg_entropy_walk(const JpegPic &pic, const uint8_t *data, size_t n, JpegEntropyWalk &w) {
    JpegSegments sg;
    w = JpegEntropyWalk();
    w.seg_error = jpeg_segment_scan(pic, data, n, sg);
    w.segs = sg.segs; w.clean = sg.bytes;
    const size_t n_blocks = (size_t)pic.n_blocks();
    JpegDevHuff tabs[6]; jpeg_device_tables(pic, tabs);
    JpegDevHuff *d_tab = exact_copy(tabs, 6);
    JpegSegment *d_segs = exact_copy(sg.segs.data(), sg.segs.size());
    // the clean bytes are read as dwords: their size is a multiple of 4 by construction
    if (sg.bytes.size() % 4) abort();
    uint32_t *d_bytes = (uint32_t *)exact_copy(sg.bytes.data(), sg.bytes.size());
    uint32_t *d_first = (uint32_t *)malloc(n_blocks ? n_blocks * 4 : 1); memset(d_first, 0xEE, n_blocks * 4);
    uint8_t *d_count = (uint8_t *)malloc(n_blocks ? n_blocks : 1); memset(d_count, 0xEE, n_blocks);
    uint32_t *d_entries = (uint32_t *)malloc(sg.n_entries ? (size_t)sg.n_entries * 4 : 1);
    const JpegScanGeom g = jpeg_scan_geom(pic);
    const uint32_t bpm = pic.ncomp == 3 ? (uint32_t)(g.hs * g.vs) + 2 : 1;
    size_t covered = 0;
    for (size_t s = 0; s < sg.segs.size(); s++) {
        const JpegSegment &seg = d_segs[s];
        long long iters = -1;
        const int dmg = jpeg_entropy_segment(g, d_tab, seg, d_bytes, d_first, d_count, d_entries, &iters);
        const uint32_t B = seg.n_mcus * bpm;
        if (iters < 0 || iters > 8ll * seg.n_bytes + 65ll * B) w.bound_ok = false;
        // entries the segment holds: those of its blocks
        uint32_t used = 0;
        for (uint32_t b = 0; b < B; b++) { int c; const uint32_t idx = jpeg_entropy_block_index(g, seg.first_mcu + b / bpm, (int)(b % bpm), &c);
            if (idx >= n_blocks) abort();
            used += d_count[idx]; }
        if (used > seg.entry_cap) w.bound_ok = false;
        if (!dmg && B && used == seg.entry_cap) w.cap_reached = true;
        w.seg_damage.push_back(dmg); w.seg_used.push_back(used); w.damaged += dmg != 0;
        covered += B;
    }
    w.covered = covered == n_blocks;
    w.first.assign(d_first, d_first + n_blocks); w.count.assign(d_count, d_count + n_blocks); w.entries.assign(d_entries, d_entries + sg.n_entries);
    free(d_tab); free(d_segs); free(d_bytes); free(d_first); free(d_count); free(d_entries);
}

// Does the walk agree with the host decoder's job list?  Blocks of undamaged segments must hold the same (position, level) lists; a damaged segment
// must hold the host's lists up to some block and nothing from there on (when `strict_host` the host's own lists say where: host damage empties
// everything behind it, so this is only meaningful for the first damaged segment).  Returns the number of blocks that break this.
inline long jpeg_entropy_compare(const JpegPic &pic, const JpegEntropyWalk &w, const JpegJobs &host) {
    const JpegScanGeom g = jpeg_scan_geom(pic);
    const uint32_t bpm = pic.ncomp == 3 ? (uint32_t)(g.hs * g.vs) + 2 : 1;
    long bad = 0;
    for (size_t s = 0; s < w.segs.size(); s++) {
        const JpegSegment &seg = w.segs[s];
        bool empty_from_here = false;
        for (uint32_t b = 0; b < seg.n_mcus * bpm; b++) {
            int c; const uint32_t idx = jpeg_entropy_block_index(g, seg.first_mcu + b / bpm, (int)(b % bpm), &c);
            const bool same = w.count[idx] == host.count[idx] && (size_t)w.first[idx] + w.count[idx] <= w.entries.size() &&
                !memcmp(w.entries.data() + w.first[idx], host.entries.data() + host.first[idx], 4 * (size_t)w.count[idx]);
            if (!w.seg_damage[s]) { bad += !same; continue; }
            if (!empty_from_here && !same) empty_from_here = true;
            if (empty_from_here) bad += w.count[idx] != 0;
        }
    }
    return bad;
}

}  // namespace jmamd
