// tests/native/jpeg_check.cpp -- the product's MJPEG host path on the CPU: JpegSplitter, jpeg_parse_picture, jpeg_decode_scan (jpeg_syntax.cpp) and
// the reconstruction of jpeg_recon.h, whose arithmetic routines are the ones k_jpeg_recon runs.  Built with g++ by tests/test_mjpeg_host.py, which
// compares the frames with the Python restatement bit for bit.
#include "../../jmcodec_amd/csrc/jpeg_syntax.h"
#include "../../jmcodec_amd/csrc/jpeg_recon.h"
#include <cstring>
#include <string>

using namespace jmamd;
static std::string g_err;

extern "C" {
// Decodes every picture of a stream fed in chunks of `chunk` bytes (0: all at once) into tight NV12 frames, one after another in out; dims gets
// (width, height) per frame.  Returns the number of frames, -1 when a picture uses a refused feature (jc_error says which), -2 when out is too small.
// *errors counts damaged pictures.
long jc_decode(const uint8_t *data, long n, long chunk, uint8_t *out, long cap, int *dims, int max_frames, int *errors) {
    JpegSplitter sp; JpegTables tab; JpegJobs jobs;
    long frames = 0, used = 0; bool refused = false, full = false;
    *errors = 0; g_err.clear();
    auto sink = [&](const uint8_t *p, size_t len, bool truncated) {
        if (refused || full) return;
        JpegPic pic; bool refuse = false;
        const std::string e = jpeg_parse_picture(p, len, tab, pic, &refuse);
        if (!e.empty()) { g_err = e; if (refuse) refused = true; else (*errors)++; return; }
        if (truncated) (*errors)++;
        const std::string e2 = jpeg_decode_scan(pic, p, len, jobs);
        if (!e2.empty()) { g_err = e2; (*errors)++; }
        std::vector<uint8_t> f;
        jpeg_reconstruct_host(pic.sampling, pic.y_bw, pic.y_bh, pic.c_bw, pic.c_bh, jobs.first.data(), jobs.count.data(), jobs.entries.data(),
                              jobs.entries.size(), pic.q, pic.disp_w(), pic.disp_h(), f);
        if (frames >= max_frames || used + (long)f.size() > cap) { full = true; return; }
        memcpy(out + used, f.data(), f.size()); used += (long)f.size();
        dims[2 * frames] = pic.disp_w(); dims[2 * frames + 1] = pic.disp_h(); frames++;
    };
    if (chunk <= 0) chunk = n > 0 ? n : 1;
    for (long o = 0; o < n; o += chunk) sp.feed(data + o, (size_t)(n - o < chunk ? n - o : chunk), sink);
    if (sp.flush(sink)) (*errors)++;
    return refused ? -1 : (full ? -2 : frames);
}
const char *jc_error() { return g_err.c_str(); }
// the product's Annex K.3 tables: cls 0 DC / 1 AC, id 0 luminance / 1 chrominance; returns the number of values
int jc_std_table(int cls, int id, uint8_t bits[16], uint8_t vals[256]) {
    const uint8_t *b = cls ? (id ? kJpegStdAcChromaBits : kJpegStdAcLumaBits) : (id ? kJpegStdDcChromaBits : kJpegStdDcLumaBits);
    const uint8_t *v = cls ? (id ? kJpegStdAcChromaVals : kJpegStdAcLumaVals) : (id ? kJpegStdDcChromaVals : kJpegStdDcLumaVals);
    int n = 0; for (int i = 0; i < 16; i++) { bits[i] = b[i]; n += b[i]; }
    memcpy(vals, v, (size_t)n);
    return n;
}
int jc_idct_m(int k, int n) { return jpeg_m(k, n); }
}
