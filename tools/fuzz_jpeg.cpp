// tools/fuzz_jpeg.cpp -- the MJPEG host path (JpegSplitter, jpeg_parse_picture, jpeg_decode_scan, the reconstruction of jpeg_recon.h) on mutated
// streams, built with AddressSanitizer / UBSan (host sanitizers; `make -C tools fuzz_jpeg`).  Nothing here touches a device.
//   fuzz_jpeg <stream.mjpeg> <seed> <trials>
// Trial 0 feeds the stream as it is; the others flip, insert, delete and truncate bytes and feed the result in random chunks.
#include "../jmcodec_amd/csrc/jpeg_syntax.h"
#include "../jmcodec_amd/csrc/jpeg_recon.h"
#include <cstdio>
#include <cstdlib>
#include <random>

using namespace jmamd;

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: fuzz_jpeg <stream> <seed> <trials>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> src; { uint8_t buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) src.insert(src.end(), buf, buf + k); }
    fclose(f);
    std::mt19937 rng((unsigned)atoi(argv[2]));
    const int trials = atoi(argv[3]);
    long pictures = 0, damaged = 0, refused = 0;
    for (int t = 0; t < trials; t++) {
        std::vector<uint8_t> d = src;
        if (t > 0 && !d.empty()) {
            const int n_mut = 1 + (int)(rng() % 8);
            for (int m = 0; m < n_mut && !d.empty(); m++) {
                const size_t at = rng() % d.size();
                switch (rng() % 5) {
                case 0: d[at] ^= (uint8_t)(1u << (rng() % 8)); break;
                case 1: d[at] = (uint8_t)rng(); break;
                case 2: d.insert(d.begin() + (long)at, (uint8_t)(rng() % 2 ? 0xFF : rng())); break;
                case 3: d.erase(d.begin() + (long)at); break;
                default: if (rng() % 4 == 0) d.resize(at); break;
                }
            }
        }
        JpegSplitter sp; JpegTables tab; JpegJobs jobs; std::vector<uint8_t> frame;
        auto sink = [&](const uint8_t *p, size_t len, bool) {
            JpegPic pic; bool refuse = false;
            if (!jpeg_parse_picture(p, len, tab, pic, &refuse).empty()) { (refuse ? refused : damaged)++; return; }
            if (pic.width > 1024 || pic.height > 1024) return;           // (a mutated size field: keep the trial short)
            if (!jpeg_decode_scan(pic, p, len, jobs).empty()) damaged++;
            jpeg_reconstruct_host(pic.sampling, pic.y_bw, pic.y_bh, pic.c_bw, pic.c_bh, jobs.first.data(), jobs.count.data(), jobs.entries.data(),
                                  jobs.entries.size(), pic.q, pic.disp_w(), pic.disp_h(), frame);
            pictures++;
        };
        for (size_t o = 0; o < d.size();) { const size_t k = std::min(d.size() - o, (size_t)(t % 3 == 0 ? d.size() : 1 + rng() % 300)); sp.feed(d.data() + o, k, sink); o += k; }
        sp.flush(sink);
    }
    printf("ok: %d trials, %ld pictures decoded, %ld damaged, %ld refused\n", trials, pictures, damaged, refused);
    return 0;
}
