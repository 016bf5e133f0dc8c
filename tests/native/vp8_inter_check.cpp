// tests/native/vp8_inter_check.cpp -- the product's VP8 host path with option vp8_inter on the CPU: Vp8Splitter, vp8_read_tag, vp8_decode_frame with the
// stream's Vp8State, vp8_validate_jobs (vp8_syntax.cpp) and the lane routines of vp8_recon.h playing k_vp8_inter, k_vp8_recon and k_vp8_filter in the
// kernels' order, with the reference rule of vp8_decoder.cpp (RFC 6386 9.7) on shared surfaces.  Built with g++ by tests/test_vp8_inter_host.py, which
// compares frames, counts and tables with the Python restatement (tests/vp8_inter_ref.py) bit for bit.
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
    std::vector<std::shared_ptr<Surface>> out, all;
    std::shared_ptr<Surface> ref[3];          // last, golden, altref
    Vp8State state;
    long long errors = 0, key_frames = 0, inter_frames = 0, hidden = 0, empty = 0, bpred = 0, skipped = 0, job_bytes = 0;
    long long golden = 0, altref = 0, split = 0, intra_in_inter = 0;
    uint64_t digest = 1469598103934665603ull;
    int width = 0, height = 0;
    bool refused = false, allow_inter = true;
    void hash(const void *p, size_t n) { const uint8_t *b = (const uint8_t *)p; for (size_t i = 0; i < n; i++) { digest ^= b[i]; digest *= 1099511628211ull; } }
    void frame(const uint8_t *p, size_t n, bool truncated) {
        if (refused) return;
        if (n == 0) { empty++; return; }
        Vp8Pic pic;
        const std::string e = vp8_read_tag(p, n, key_frames == 0, pic.tag, allow_inter);
        if (!e.empty()) { g_err = e; refused = true; return; }
        if (pic.tag.key) { width = pic.tag.width; height = pic.tag.height; } else { pic.tag.width = width; pic.tag.height = height; }
        vp8_decode_frame(p, n, pic, &state);
        const std::string v = vp8_validate_jobs(pic);
        if (!v.empty()) { g_err = v; refused = true; return; }
        if (pic.damaged || truncated) errors++;
        if (pic.tag.key) key_frames++; else inter_frames++;
        if (!pic.tag.show) hidden++;
        bpred += pic.bpred_mbs; skipped += pic.skipped_mbs;
        job_bytes += (long long)(pic.mbs.size() * sizeof(Vp8Mb) + pic.entries.size() * 4 + pic.split.size() * sizeof(Vp8SplitMv));
        hash(pic.mbs.data(), pic.mbs.size() * sizeof(Vp8Mb)); hash(pic.entries.data(), pic.entries.size() * 4); hash(pic.split.data(), pic.split.size() * sizeof(Vp8SplitMv));
        if (!pic.tag.key) { golden += pic.golden_mbs; altref += pic.alt_mbs; split += pic.split_mbs; intra_in_inter += pic.intra_mbs; }
        auto cur = std::make_shared<Surface>();
        cur->W = pic.mb_w * 16; cur->H = pic.mb_h * 16; cur->w = (pic.tag.width + 1) & ~1; cur->h = (pic.tag.height + 1) & ~1;
        cur->s.assign((size_t)cur->W * cur->H * 3 / 2, 128);
        Vp8PicParams pp = {};
        pp.surf = cur->s.data(); pp.pitch = cur->W; pp.chroma_offset = cur->W * cur->H; pp.mb_w = pic.mb_w; pp.mb_h = pic.mb_h;
        pp.n_entries = (int)pic.entries.size(); pp.filter_type = pic.filter_type; pp.sharpness = pic.sharpness; pp.filtered = pic.filtered;
        pp.mbs = pic.mbs.data(); pp.entries = pic.entries.data();
        memcpy(pp.dq, pic.dq, sizeof pp.dq);
        if (!pic.tag.key) {
            pp.inter = 1; pp.interp = pic.tag.version == 0 ? 0 : 1; pp.n_intra = pic.intra_mbs; pp.n_split = (int)pic.split.size();
            pp.split = pic.split.data();
            for (int k = 0; k < 3; k++) pp.ref[k] = ref[k] && ref[k]->W == cur->W && ref[k]->H == cur->H ? ref[k]->s.data() : nullptr;
        }
        vp8_inter_host(pp);
        vp8_reconstruct_host(pp);
        vp8_filter_host(pp);
        // RFC 6386 9.7: copies from the references as they were, then the refreshes
        if (pic.tag.key) ref[0] = ref[1] = ref[2] = cur;
        else {
            const auto last = ref[0], gold = ref[1], alt = ref[2];
            if (pic.copy_to_alt == 1) ref[2] = last; else if (pic.copy_to_alt == 2) ref[2] = gold;
            if (pic.copy_to_golden == 1) ref[1] = last; else if (pic.copy_to_golden == 2) ref[1] = alt;
            if (pic.refresh_golden) ref[1] = cur;
            if (pic.refresh_alt) ref[2] = cur;
            if (pic.refresh_last) ref[0] = cur;
        }
        all.push_back(cur);
        if (pic.tag.show) out.push_back(cur);
    }
};
}  // namespace

extern "C" {
// As v8c_decode of vp8_check.cpp, with inter frames (inter: 0 = refuse them, as a handle without the option).  every != 0: hidden frames are handed out
// too.  stats[16]: errors, key frames, inter frames, hidden, empty, B_PRED macroblocks, skipped macroblocks, job bytes, golden references, altref
// references, split macroblocks, intra macroblocks of inter frames, job digest (FNV-1a over records, entries and split vectors).
long v8i_decode(const uint8_t *data, long n, long chunk, int inter, int every, uint8_t *out, long cap, int *dims, int max_frames, long long *stats) {
    Vp8Splitter sp; Host h;
    h.allow_inter = inter != 0;
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
    stats[0] = h.errors; stats[1] = h.key_frames; stats[2] = h.inter_frames; stats[3] = h.hidden; stats[4] = h.empty; stats[5] = h.bpred; stats[6] = h.skipped;
    stats[7] = h.job_bytes; stats[8] = h.golden; stats[9] = h.altref; stats[10] = h.split; stats[11] = h.intra_in_inter; stats[12] = (long long)h.digest;
    if (h.refused) return -1;
    long used = 0, frames = 0;
    for (auto &f : every ? h.all : h.out) {
        const long bytes = (long)f->w * f->h * 3 / 2;
        if (frames >= max_frames || used + bytes > cap) return -2;
        uint8_t *d = out + used;
        for (int y = 0; y < f->h; y++) memcpy(d + (size_t)y * f->w, f->s.data() + (size_t)y * f->W, (size_t)f->w);
        for (int y = 0; y < f->h / 2; y++) memcpy(d + (size_t)f->w * f->h + (size_t)y * f->w, f->s.data() + (size_t)f->W * f->H + (size_t)y * f->W, (size_t)f->w);
        dims[2 * frames] = f->w; dims[2 * frames + 1] = f->h; frames++; used += bytes;
    }
    return frames;
}
const char *v8i_error() { return g_err.c_str(); }
// One n x n block predicted by the lane routines from a w x h plane (w, h multiples of 16; the plane serves as luma and, interleaved with itself, as
// chroma): plane 0 luma 16x16 at macroblock (mbx, mby) with vector (mvx, mvy); interp 0 six-tap, 1 bilinear.  out: 16 x 16 luma samples then 8 x 8 U.
// split != 0: the same vector through the 24-region path.
void v8i_predict(const uint8_t *plane, int w, int h, int mbx, int mby, int mvx, int mvy, int cmvx, int cmvy, int interp, int split, uint8_t *out) {
    std::vector<uint8_t> ref((size_t)w * h * 3 / 2), cur((size_t)w * h * 3 / 2, 0);
    memcpy(ref.data(), plane, (size_t)w * h);
    for (int y = 0; y < h / 2; y++) for (int x = 0; x < w / 2; x++) ref[(size_t)w * h + (size_t)y * w + 2 * x] = ref[(size_t)w * h + (size_t)y * w + 2 * x + 1] = plane[(size_t)y * w + x];
    Vp8Mb mb; memset(&mb, 0, sizeof mb);
    Vp8InterInfo ii; memset(&ii, 0, sizeof ii);
    ii.ref = 1; ii.mvx = (int16_t)mvx; ii.mvy = (int16_t)mvy; ii.cmvx = (int16_t)cmvx; ii.cmvy = (int16_t)cmvy; ii.split = split ? 4 : 0;
    mb.flags = VP8_MB_INTER; mb.mvmode = split ? VP8_MV_SPLIT : VP8_MV_NEW; mb.ymode = split ? VP8_B_PRED : VP8_DC_PRED;
    memcpy(mb.bmodes, &ii, sizeof ii);
    Vp8SplitMv sv;
    for (auto &v : sv.y) { v[0] = (int16_t)mvx; v[1] = (int16_t)mvy; }
    for (auto &v : sv.c) { v[0] = (int16_t)cmvx; v[1] = (int16_t)cmvy; }
    std::vector<Vp8Mb> mbs((size_t)(w / 16) * (h / 16));
    for (auto &m : mbs) memset(&m, 0, sizeof m);
    mbs[(size_t)mby * (w / 16) + mbx] = mb;
    Vp8PicParams pp = {};
    pp.surf = cur.data(); pp.pitch = w; pp.chroma_offset = w * h; pp.mb_w = w / 16; pp.mb_h = h / 16; pp.mbs = mbs.data();
    pp.inter = 1; pp.interp = interp; pp.ref[0] = ref.data(); pp.split = &sv; pp.n_split = 1;
    vp8_inter_host(pp);
    for (int y = 0; y < 16; y++) memcpy(out + 16 * y, cur.data() + (size_t)(mby * 16 + y) * w + mbx * 16, 16);
    for (int y = 0; y < 8; y++) for (int x = 0; x < 8; x++) out[256 + 8 * y + x] = cur[(size_t)w * h + (size_t)(mby * 8 + y) * w + 2 * (mbx * 8 + x)];
}
// byte i of table `which`, -1 past its end: 0 ymode probabilities, 1 chroma mode probabilities, 2 sub-block mode probabilities, 3 mode contexts, 4 sub_mv_ref
// probabilities, 5 split probabilities, 6 default vector probabilities, 7 vector update probabilities, 8 split tables, 9..13 the trees (luma mode, mv_ref,
// sub_mv_ref, split, short vector; as signed bytes + 128), 14 + 16 k + f (k 0 six-tap, 1 bilinear; f 0..7): the taps of fraction f, + 128
int v8i_table(int which, long i) {
    const uint8_t *t = nullptr; long n = 0;
    switch (which) {
    case 0: t = kVp8YmodeProb; n = sizeof kVp8YmodeProb; break;
    case 1: t = kVp8UvModeProb; n = sizeof kVp8UvModeProb; break;
    case 2: t = kVp8BmodeProb; n = sizeof kVp8BmodeProb; break;
    case 3: t = &kVp8ModeContexts[0][0]; n = sizeof kVp8ModeContexts; break;
    case 4: t = &kVp8SubMvRefProbs[0][0]; n = sizeof kVp8SubMvRefProbs; break;
    case 5: t = kVp8SplitProbs; n = sizeof kVp8SplitProbs; break;
    case 6: t = &kVp8MvDefaultProbs[0][0]; n = sizeof kVp8MvDefaultProbs; break;
    case 7: t = &kVp8MvUpdateProbs[0][0]; n = sizeof kVp8MvUpdateProbs; break;
    case 8: t = &kVp8Splits[0][0]; n = sizeof kVp8Splits; break;
    case 9: t = (const uint8_t *)kVp8YmodeTree; n = sizeof kVp8YmodeTree; break;
    case 10: t = (const uint8_t *)kVp8MvRefTree; n = sizeof kVp8MvRefTree; break;
    case 11: t = (const uint8_t *)kVp8SubMvRefTree; n = sizeof kVp8SubMvRefTree; break;
    case 12: t = (const uint8_t *)kVp8SplitTree; n = sizeof kVp8SplitTree; break;
    case 13: t = (const uint8_t *)kVp8SmallMvTree; n = sizeof kVp8SmallMvTree; break;
    }
    if (which >= 14 && which < 46) {
        if (i < 0 || i >= 6) return -1;
        int taps[6];
        vp8_taps((which - 14) >> 4, (which - 14) & 7, taps);
        return taps[i] + 128;
    }
    if (!t || i < 0 || i >= n) return -1;
    return which >= 9 && which <= 13 ? (int)(int8_t)t[i] + 128 : t[i];
}
}
