// tests/native/mpeg2_check.cpp -- the product's MPEG-2 host path on the CPU: Mpeg2Splitter, mpeg2_decode_picture (mpeg2_syntax.cpp) and the
// reconstruction of mpeg2_recon.h, whose arithmetic routines are the ones k_mpeg2_recon runs, with the anchor and display-order rules of
// INTEGRATION.md "MPEG-2".  Built with g++ by tests/test_mpeg2_host.py, which compares the frames with the Python restatement bit for bit, and the
// tables with the restatement's.
#include "../../jmcodec_amd/csrc/mpeg2_syntax.h"
#include "../../jmcodec_amd/csrc/mpeg2_recon.h"
#include <cstring>
#include <memory>
#include <string>

using namespace jmamd;
static std::string g_err;

namespace {
struct Surface { std::vector<uint8_t> s; int w = 0, h = 0, W = 0, H = 0; };      // NV12, pitch = W (coded width); w x h: the display size
struct Host {
    std::shared_ptr<Surface> anchor[2]; bool shown = true;
    Mpeg2Seq seq; bool have_seq = false;
    std::vector<std::shared_ptr<Surface>> out;
    int errors = 0, dropped = 0, clamped = 0; bool refused = false;
    void show() { if (anchor[1] && !shown) { out.push_back(anchor[1]); shown = true; } }
    void picture(Mpeg2Pic &pic) {
        if (refused) return;
        if (!pic.have_ext) { errors++; return; }
        const Mpeg2Seq &s = pic.seq;
        if (have_seq && (s.width != seq.width || s.height != seq.height || s.progressive_sequence != seq.progressive_sequence)) {
            show(); anchor[0].reset(); anchor[1].reset(); }
        seq = s; have_seq = true;
        if ((pic.type == 2 && !anchor[1]) || (pic.type == 3 && (!anchor[0] || !anchor[1]))) { dropped++; return; }
        Mpeg2Jobs jobs; bool refuse = false;
        const std::string e = mpeg2_decode_picture(pic, jobs, &refuse);
        if (!e.empty()) { g_err = e; if (refuse) { refused = true; return; } errors++; }
        if (jobs.clamped) { clamped += jobs.clamped; errors++; }
        auto cur = std::make_shared<Surface>();
        cur->W = s.mb_w() * 16; cur->H = s.mb_h() * 16; cur->w = (s.width + 1) & ~1; cur->h = (s.height + 1) & ~1;
        cur->s.assign((size_t)cur->W * cur->H * 3 / 2, 0);
        Mpeg2PicParams pp = {};
        pp.surf = cur->s.data(); pp.pitch = cur->W; pp.chroma_offset = cur->W * cur->H; pp.mb_w = s.mb_w(); pp.mb_h = s.mb_h();
        pp.ref[0] = pic.type == 2 ? anchor[1]->s.data() : (pic.type == 3 ? anchor[0]->s.data() : nullptr);
        pp.ref[1] = pic.type == 3 ? anchor[1]->s.data() : nullptr;
        pp.n_entries = (int)jobs.entries.size(); pp.dc_mult = 8 >> pic.intra_dc_precision;
        pp.mbs = jobs.mbs.data(); pp.entries = jobs.entries.data();
        memcpy(pp.w, s.w, sizeof pp.w);
        mpeg2_reconstruct_host(pp);
        if (pic.type == 3) out.push_back(cur);
        else { show(); anchor[0] = anchor[1]; anchor[1] = cur; shown = false; }
    }
};
}  // namespace

extern "C" {
// Decodes a stream fed in chunks of `chunk` bytes (0: all at once, -1: one start-code unit per call) into tight NV12 display frames, one after
// another in out; dims gets (width, height) per frame.  Returns the number of frames, -1 when the stream uses a refused feature (m2c_error says
// which), -2 when out is too small.  stats: errors, dropped pictures, clamped macroblocks.
long m2c_decode(const uint8_t *data, long n, long chunk, uint8_t *out, long cap, int *dims, int max_frames, int *stats) {
    Mpeg2Splitter sp; Host h;
    g_err.clear();
    auto sink = [&](Mpeg2Pic &p) { h.picture(p); };
    if (chunk < 0) {
        long o = 0;
        while (o < n) {
            long e = o + 3;
            while (e + 3 <= n && !(data[e] == 0 && data[e + 1] == 0 && data[e + 2] == 1)) e++;
            if (e + 3 > n) e = n;
            sp.feed(data + o, (size_t)(e - o), sink); o = e;
        }
    } else {
        if (chunk == 0) chunk = n > 0 ? n : 1;
        for (long o = 0; o < n; o += chunk) sp.feed(data + o, (size_t)(n - o < chunk ? n - o : chunk), sink);
    }
    sp.flush(sink);
    h.show();
    stats[0] = h.errors + (int)sp.damaged_headers; stats[1] = h.dropped; stats[2] = h.clamped;
    if (sp.refused()) { g_err = sp.error(); return -1; }
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
const char *m2c_error() { return g_err.c_str(); }
// entry i of table `which` (mpeg2_table): code, length, a, b; returns the table's size
int m2c_table(int which, int i, int *v) {
    int n; const Mpeg2Vlc *t = mpeg2_table(which, &n);
    if (t && i >= 0 && i < n) { v[0] = t[i].code; v[1] = t[i].len; v[2] = t[i].a; v[3] = t[i].b; }
    return n;
}
int m2c_scan(int alt, int k) { return kMpeg2Scan[alt & 1][k & 63]; }
int m2c_default_intra(int k) { return kMpeg2DefaultIntra[k & 63]; }
int m2c_quantiser_scale(int type, int code) { return mpeg2_quantiser_scale(type, code); }
int m2c_idct_m(int k, int n) { return jpeg_m(k, n); }
// the product's IDCT on n blocks of 64 coefficients F[v][u] -> 64 residuals each
void m2c_idct(const int *F, int *out, long n) {
    for (long b = 0; b < n; b++) {
        int g[64];
        for (int u = 0; u < 8; u++) { int col[8], o[8]; for (int v = 0; v < 8; v++) col[v] = F[b * 64 + v * 8 + u]; jpeg_pass1(col, o);
            for (int y = 0; y < 8; y++) g[y * 8 + u] = o[y]; }
        for (int y = 0; y < 8; y++) mpeg2_pass2(g + y * 8, out + b * 64 + y * 8);
    }
}
}
