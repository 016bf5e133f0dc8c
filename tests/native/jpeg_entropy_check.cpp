// tests/native/jpeg_entropy_check.cpp -- option jpeg_device_entropy on the CPU: the segmenter (jpeg_segment_scan) and the device routine
// (jpeg_entropy_segment, the code k_jpeg_entropy runs) walked over every segment of a picture (jpeg_entropy_walk.h), next to the host decoder
// jpeg_decode_scan.  Built with g++ by tests/test_mjpeg_entropy_host.py, which compares per block the lists of (position, level).
#include "jpeg_entropy_walk.h"

using namespace jmamd;
static std::string g_err;
static JpegTables g_tab;

extern "C" {
void jec_reset() { g_tab = JpegTables(); g_err.clear(); }
const char *jec_error() { return g_err.c_str(); }

// The host decoder's job list of one picture (tables persist from call to call until jec_reset).  info: [0] blocks, [1] entries, [2] error (0 / 1).
// Returns 0, -1 when the headers cannot be read, -2 when a buffer is too small.
long jec_host(const uint8_t *data, long n, uint32_t *first, uint8_t *count, uint32_t *entries, long blocks_cap, long entries_cap, int *info) {
    JpegPic pic; bool refuse = false; JpegJobs jobs;
    const std::string e = jpeg_parse_picture(data, (size_t)n, g_tab, pic, &refuse);
    if (!e.empty()) { g_err = e; return -1; }
    const std::string e2 = jpeg_decode_scan(pic, data, (size_t)n, jobs);
    g_err = e2;
    if ((long)jobs.first.size() > blocks_cap || (long)jobs.entries.size() > entries_cap) return -2;
    if (!jobs.first.empty()) { memcpy(first, jobs.first.data(), jobs.first.size() * 4); memcpy(count, jobs.count.data(), jobs.count.size()); }
    if (!jobs.entries.empty()) memcpy(entries, jobs.entries.data(), jobs.entries.size() * 4);
    info[0] = (int)jobs.first.size(); info[1] = (int)jobs.entries.size(); info[2] = !e2.empty();
    return 0;
}

// The walk of one picture.  segs: 6 words per segment (JpegSegment); seg_damage: per segment the kind of damage; clean: the clean bytes.
// info: [0] blocks, [1] segments, [2] entry capacity in all, [3] damaged segments, [4] the segmenter complained, [5] iteration and capacity bounds
// held, [6] an undamaged segment filled its capacity exactly, [7] every block belongs to exactly one segment's range, [8] blocks that disagree with
// the host decoder's list of the same bytes (jpeg_entropy_compare), [9] the host decoder complained, [10] clean bytes, [11] entries in the host's list.
long jec_walk(const uint8_t *data, long n, uint32_t *first, uint8_t *count, uint32_t *entries, long blocks_cap, long entries_cap,
              uint32_t *segs, int *seg_damage, long segs_cap, uint8_t *clean, long clean_cap, int *info) {
    JpegPic pic; bool refuse = false; JpegJobs jobs; JpegEntropyWalk w;
    const std::string e = jpeg_parse_picture(data, (size_t)n, g_tab, pic, &refuse);
    if (!e.empty()) { g_err = e; return -1; }
    jpeg_entropy_walk(pic, data, (size_t)n, w);
    const std::string e2 = jpeg_decode_scan(pic, data, (size_t)n, jobs);
    g_err = w.seg_error.empty() ? e2 : w.seg_error;
    if ((long)w.first.size() > blocks_cap || (long)w.entries.size() > entries_cap || (long)w.segs.size() > segs_cap || (long)w.clean.size() > clean_cap) return -2;
    if (!w.first.empty()) { memcpy(first, w.first.data(), w.first.size() * 4); memcpy(count, w.count.data(), w.count.size()); }
    if (!w.entries.empty()) memcpy(entries, w.entries.data(), w.entries.size() * 4);
    if (!w.segs.empty()) { memcpy(segs, w.segs.data(), w.segs.size() * sizeof(JpegSegment)); memcpy(seg_damage, w.seg_damage.data(), w.segs.size() * sizeof(int)); }
    if (!w.clean.empty()) memcpy(clean, w.clean.data(), w.clean.size());
    info[0] = (int)w.first.size(); info[1] = (int)w.segs.size(); info[2] = (int)w.entries.size(); info[3] = w.damaged; info[4] = !w.seg_error.empty();
    info[5] = w.bound_ok; info[6] = w.cap_reached; info[7] = w.covered; info[8] = (int)jpeg_entropy_compare(pic, w, jobs); info[9] = !e2.empty();
    info[10] = (int)w.clean.size(); info[11] = (int)jobs.entries.size();
    return 0;
}
int jec_guard() { return kJpegSegGuard; }
unsigned jec_capacity(unsigned n_bytes, unsigned n_blocks) { return jpeg_entropy_capacity(n_bytes, n_blocks); }
}
