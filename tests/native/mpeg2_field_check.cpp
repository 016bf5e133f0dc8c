// tests/native/mpeg2_field_check.cpp -- the product's MPEG-2 host path with option mpeg2_field_pictures on, on the CPU: Mpeg2Splitter with its
// switch set, mpeg2_decode_picture and mpeg2_reconstruct_host (the arithmetic k_mpeg2_recon runs), with the field pairing, reference field and
// lone-field rules of INTEGRATION.md "MPEG-2".  Built with g++ by tests/test_mpeg2_field_host.py, which compares the frames with the numpy
// restatement (tests/mpeg2_field_ref.py) bit for bit.  tests/native/mpeg2_check.cpp stays the check of the default-constructed splitter.
#include "mpeg2_field_host.h"

extern "C" {
// As m2c_decode of mpeg2_check.cpp, with the splitter's switch on.  stats: errors, dropped pictures, clamped macroblocks, lone fields, field
// pictures, dual-prime records, 16x8 records.
long m2f_decode(const uint8_t *data, long n, long chunk, uint8_t *out, long cap, int *dims, int max_frames, int *stats) {
    Mpeg2Splitter sp; Host h;
    sp.field_pictures = true;
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
    h.close_pending();
    h.show();
    stats[0] = h.errors + (int)sp.damaged_headers; stats[1] = h.dropped; stats[2] = h.clamped; stats[3] = h.lone; stats[4] = h.fields;
    stats[5] = h.n_dual; stats[6] = h.n_16x8;
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
const char *m2f_error() { return g_err.c_str(); }
// entry i of table `which` (mpeg2_table): code, length, a, b; returns the table's size
int m2f_table(int which, int i, int *v) {
    int n; const Mpeg2Vlc *t = mpeg2_table(which, &n);
    if (t && i >= 0 && i < n) { v[0] = t[i].code; v[1] = t[i].len; v[2] = t[i].a; v[3] = t[i].b; }
    return n;
}
}
