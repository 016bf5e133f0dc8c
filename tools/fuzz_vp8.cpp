// tools/fuzz_vp8.cpp -- the VP8 host path (Vp8Splitter, vp8_read_tag, vp8_decode_frame, vp8_validate_jobs, then the lane routines of vp8_recon.h in
// the kernels' wavefront order over surfaces of exactly the device's extent) on mutated streams, built with AddressSanitizer / UBSan (host
// sanitizers; `make -C tools fuzz_vp8_asan`).  Nothing here touches a device.
//   fuzz_vp8_asan <stream.ivf> <seed> <trials>
// Trial 0 feeds the stream as it is; the others flip, insert, delete and truncate bytes and feed the result in random chunks.  A job list the parser
// wrote must always validate: anything else ends the program with status 1.
#include "../jmcodec_amd/csrc/vp8_syntax.h"
#include "../jmcodec_amd/csrc/vp8_recon.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

using namespace jmamd;

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: fuzz_vp8_asan <stream> <seed> <trials>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> src; { uint8_t buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) src.insert(src.end(), buf, buf + k); }
    fclose(f);
    std::mt19937 rng((unsigned)atoi(argv[2]));
    const int trials = atoi(argv[3]);
    long pictures = 0, damaged = 0, refused = 0, empty = 0; int bad = 0;
    for (int t = 0; t < trials; t++) {
        std::vector<uint8_t> d = src;
        if (t > 0 && !d.empty()) {
            const int n_mut = 1 + (int)(rng() % 8);
            for (int m = 0; m < n_mut && !d.empty(); m++) {
                const size_t at = rng() % d.size();
                switch (rng() % 5) {
                case 0: d[at] ^= (uint8_t)(1u << (rng() % 8)); break;
                case 1: d[at] = (uint8_t)rng(); break;
                case 2: d.insert(d.begin() + (long)at, (uint8_t)(rng() % 2 ? 0x00 : rng())); break;
                case 3: d.erase(d.begin() + (long)at); break;
                default: if (rng() % 4 == 0) d.resize(at); break;
                }
            }
        }
        Vp8Splitter sp; long keys = 0; bool stop = false;
        auto sink = [&](const uint8_t *p, size_t n, bool truncated) {
            if (stop) return;
            if (n == 0) { empty++; return; }
            std::unique_ptr<uint8_t[]> frame(new uint8_t[n]);            // exactly the frame: the bool decoders may not read beyond it
            memcpy(frame.get(), p, n);
            Vp8Pic pic;
            if (!vp8_read_tag(frame.get(), n, keys == 0, pic.tag).empty()) { refused++; stop = true; return; }
            if (pic.tag.width > 1024 || pic.tag.height > 1024) return;   // (a mutated size field: keep the trial short)
            vp8_decode_frame(frame.get(), n, pic);
            if (!vp8_validate_jobs(pic).empty()) { fprintf(stderr, "trial %d: the parser's own job list does not validate: %s\n", t, vp8_validate_jobs(pic).c_str()); bad = 1; return; }
            keys++; if (pic.damaged || truncated) damaged++;
            const int W = pic.mb_w * 16, H = pic.mb_h * 16;
            std::unique_ptr<uint8_t[]> surf(new uint8_t[(size_t)W * H * 3 / 2]);
            memset(surf.get(), 128, (size_t)W * H * 3 / 2);
            std::unique_ptr<uint32_t[]> entries(new uint32_t[pic.entries.size() ? pic.entries.size() : 1]);
            if (!pic.entries.empty()) memcpy(entries.get(), pic.entries.data(), pic.entries.size() * 4);
            Vp8PicParams pp = {};
            pp.surf = surf.get(); pp.pitch = W; pp.chroma_offset = W * H; pp.mb_w = pic.mb_w; pp.mb_h = pic.mb_h;
            pp.n_entries = (int)pic.entries.size(); pp.filter_type = pic.filter_type; pp.sharpness = pic.sharpness; pp.filtered = pic.filtered;
            pp.mbs = pic.mbs.data(); pp.entries = entries.get();
            memcpy(pp.dq, pic.dq, sizeof pp.dq);
            vp8_reconstruct_host(pp);
            vp8_filter_host(pp);
            pictures++;
        };
        for (size_t o = 0; o < d.size();) { const size_t k = std::min(d.size() - o, (size_t)(t % 3 == 0 ? d.size() : 1 + rng() % 300)); sp.feed(d.data() + o, k, sink); o += k; }
        sp.flush(sink);
    }
    printf("%s: %d trials, %ld pictures decoded, %ld damaged, %ld refused, %ld empty frames\n", bad ? "FAILED" : "ok", trials, pictures, damaged, refused, empty);
    return bad;
}
