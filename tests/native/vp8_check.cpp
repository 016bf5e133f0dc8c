// tests/native/vp8_check.cpp -- the product's VP8 host path on the CPU: Vp8Splitter, vp8_read_tag, vp8_decode_frame, vp8_validate_jobs
// (vp8_syntax.cpp) and the lane routines of vp8_recon.h playing k_vp8_recon and k_vp8_filter in the kernels' wavefront order, with the input and
// display rules of INTEGRATION.md "VP8".  Built with g++ by tests/test_vp8_host.py, which compares the frames with libwebp's recorded planes and with
// the Python restatement bit for bit, and the tables with the restatement's.
#include "../../jmcodec_amd/csrc/vp8_syntax.h"
#include "../../jmcodec_amd/csrc/vp8_recon.h"
#include <cstring>
#include <memory>
#include <string>

using namespace jmamd;
static std::string g_err;

namespace {
struct Surface { std::vector<uint8_t> s; int w = 0, h = 0, W = 0, H = 0; };      // NV12, pitch = W (coded width); w x h: the display size
struct Host {
    std::vector<std::shared_ptr<Surface>> out;
    long long errors = 0, key_frames = 0, hidden = 0, empty = 0, bpred = 0, skipped = 0, job_bytes = 0;
    int partitions = 0, segments = 0, filter_type = 0, color_space = 0, scale = 0;
    bool refused = false;
    void frame(const uint8_t *p, size_t n, bool truncated) {
        if (refused) return;
        if (n == 0) { empty++; return; }
        Vp8Pic pic;
        const std::string e = vp8_read_tag(p, n, key_frames == 0, pic.tag);
        if (!e.empty()) { g_err = e; refused = true; return; }
        vp8_decode_frame(p, n, pic);
        const std::string v = vp8_validate_jobs(pic);
        if (!v.empty()) { g_err = v; refused = true; return; }
        if (pic.damaged || truncated) errors++;
        key_frames++; if (!pic.tag.show) hidden++;
        partitions = pic.n_parts; filter_type = pic.filter_type; color_space = pic.color_space | pic.clamping << 1; scale = pic.tag.hscale | pic.tag.vscale << 2;
        segments = 0; for (int s = 0; s < 4; s++) segments += pic.segments_used >> s & 1;
        bpred += pic.bpred_mbs; skipped += pic.skipped_mbs; job_bytes += (long long)(pic.mbs.size() * sizeof(Vp8Mb) + pic.entries.size() * 4);
        auto cur = std::make_shared<Surface>();
        cur->W = pic.mb_w * 16; cur->H = pic.mb_h * 16; cur->w = (pic.tag.width + 1) & ~1; cur->h = (pic.tag.height + 1) & ~1;
        cur->s.assign((size_t)cur->W * cur->H * 3 / 2, 128);
        Vp8PicParams pp = {};
        pp.surf = cur->s.data(); pp.pitch = cur->W; pp.chroma_offset = cur->W * cur->H; pp.mb_w = pic.mb_w; pp.mb_h = pic.mb_h;
        pp.n_entries = (int)pic.entries.size(); pp.filter_type = pic.filter_type; pp.sharpness = pic.sharpness; pp.filtered = pic.filtered;
        pp.mbs = pic.mbs.data(); pp.entries = pic.entries.data();
        memcpy(pp.dq, pic.dq, sizeof pp.dq);
        vp8_reconstruct_host(pp);
        vp8_filter_host(pp);
        if (pic.tag.show) out.push_back(cur);
    }
};
}  // namespace

extern "C" {
// Decodes a stream fed in chunks of `chunk` bytes (0: all at once; -1: data is a list of frames, each behind a 4-byte little-endian length, fed one
// frame per call) into tight NV12 display frames, one after another in out; dims gets (width, height) per frame.  Returns the number of frames, -1
// when the stream is refused (v8c_error says why), -2 when out is too small.  stats[12]: errors, key frames, hidden frames, empty frames, partitions,
// segments, filter type, colour space | clamping << 1, scale, B_PRED macroblocks, skipped macroblocks, job bytes.
long v8c_decode(const uint8_t *data, long n, long chunk, uint8_t *out, long cap, int *dims, int max_frames, long long *stats) {
    Vp8Splitter sp; Host h;
    g_err.clear();
    auto sink = [&](const uint8_t *p, size_t len, bool truncated) { h.frame(p, len, truncated); };
    if (chunk < 0) {
        long o = 0;
        while (o + 4 <= n) {
            const long len = (long)data[o] | (long)data[o + 1] << 8 | (long)data[o + 2] << 16 | (long)data[o + 3] << 24;
            if (len < 0 || o + 4 + len > n) break;
            sp.feed(data + o + 4, (size_t)len, sink); o += 4 + len;
        }
    } else {
        if (chunk == 0) chunk = n > 0 ? n : 1;
        for (long o = 0; o < n; o += chunk) sp.feed(data + o, (size_t)(n - o < chunk ? n - o : chunk), sink);
    }
    if (sp.flush(sink)) h.errors++;
    stats[0] = h.errors; stats[1] = h.key_frames; stats[2] = h.hidden; stats[3] = h.empty; stats[4] = h.partitions; stats[5] = h.segments;
    stats[6] = h.filter_type; stats[7] = h.color_space; stats[8] = h.scale; stats[9] = h.bpred; stats[10] = h.skipped; stats[11] = h.job_bytes;
    if (h.refused) return -1;
    long used = 0, frames = 0;
    for (auto &f : h.out) {
        const long bytes = (long)f->w * f->h * 3 / 2;
        if (frames >= max_frames || used + bytes > cap) return -2;
        uint8_t *d = out + used;
        for (int y = 0; y < f->h; y++) memcpy(d + (size_t)y * f->w, f->s.data() + (size_t)y * f->W, (size_t)f->w);
        for (int y = 0; y < f->h / 2; y++) memcpy(d + (size_t)f->w * f->h + (size_t)y * f->w, f->s.data() + (size_t)f->W * f->H + (size_t)y * f->W, (size_t)f->w);
        dims[2 * frames] = f->w; dims[2 * frames + 1] = f->h; frames++; used += bytes;
    }
    return frames;
}
const char *v8c_error() { return g_err.c_str(); }
// byte i of table `which`, -1 past its end: 0 dc_q, 1 ac_q (16-bit entries, low byte first), 2 default coefficient probabilities, 3 coefficient update
// probabilities, 4 key-frame luma mode probabilities, 5 chroma mode probabilities, 6 sub-block mode probabilities, 7..11 the trees (luma, chroma,
// sub-block, segment, token; as signed bytes + 128), 12 bands, 13 zig-zag, 14 category probabilities (6 x 12), 15 category bases
int v8c_table(int which, long i) {
    const uint8_t *t = nullptr; long n = 0;
    switch (which) {
    case 0: t = kVp8DcQ; n = sizeof kVp8DcQ; break;
    case 1: t = (const uint8_t *)kVp8AcQ; n = sizeof kVp8AcQ; break;
    case 2: t = &kVp8CoefProbs[0][0][0][0]; n = sizeof kVp8CoefProbs; break;
    case 3: t = &kVp8CoefUpdateProbs[0][0][0][0]; n = sizeof kVp8CoefUpdateProbs; break;
    case 4: t = kVp8KfYmodeProb; n = sizeof kVp8KfYmodeProb; break;
    case 5: t = kVp8KfUvModeProb; n = sizeof kVp8KfUvModeProb; break;
    case 6: t = &kVp8KfBmodeProbs[0][0][0]; n = sizeof kVp8KfBmodeProbs; break;
    case 7: t = (const uint8_t *)kVp8KfYmodeTree; n = sizeof kVp8KfYmodeTree; break;
    case 8: t = (const uint8_t *)kVp8UvModeTree; n = sizeof kVp8UvModeTree; break;
    case 9: t = (const uint8_t *)kVp8BmodeTree; n = sizeof kVp8BmodeTree; break;
    case 10: t = (const uint8_t *)kVp8SegmentTree; n = sizeof kVp8SegmentTree; break;
    case 11: t = (const uint8_t *)kVp8CoefTree; n = sizeof kVp8CoefTree; break;
    case 12: t = kVp8CoefBands; n = sizeof kVp8CoefBands; break;
    case 13: t = kVp8Zigzag; n = sizeof kVp8Zigzag; break;
    case 14: t = &kVp8CatProbs[0][0]; n = sizeof kVp8CatProbs; break;
    case 15: t = kVp8CatBase; n = sizeof kVp8CatBase; break;
    }
    if (!t || i < 0 || i >= n) return -1;
    return which >= 7 && which <= 11 ? (int)(int8_t)t[i] + 128 : t[i];
}
}
