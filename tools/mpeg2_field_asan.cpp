// tools/mpeg2_field_asan.cpp -- the MPEG-2 host path with option mpeg2_field_pictures on (the splitter's switch set: field pictures, 16x8 motion
// compensation, dual prime, field pairing and lone fields -- tests/native/mpeg2_field_host.h) on mutated streams, built with AddressSanitizer /
// UBSan (host sanitizers; `make -C tools mpeg2_field_asan`).  Nothing here touches a device.
//   mpeg2_field_asan <stream.m2v> <seed> <trials>
// Trial 0 feeds the stream as it is; the others flip, insert, delete and truncate bytes and feed the result in random chunks.
#include "../tests/native/mpeg2_field_host.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: mpeg2_field_asan <stream> <seed> <trials>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> src; { uint8_t buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) src.insert(src.end(), buf, buf + k); }
    fclose(f);
    std::mt19937 rng((unsigned)atoi(argv[2]));
    const int trials = atoi(argv[3]);
    long pictures = 0, fields = 0, errors = 0, refused = 0, dropped = 0, clamped = 0, lone = 0, dual = 0, m16x8 = 0;
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
        Mpeg2Splitter sp; Host h;
        sp.field_pictures = true; h.max_mb = 64;
        auto sink = [&](Mpeg2Pic &pic) { h.picture(pic); };
        for (size_t o = 0; o < d.size();) { const size_t k = std::min(d.size() - o, (size_t)(t % 3 == 0 ? d.size() : 1 + rng() % 300)); sp.feed(d.data() + o, k, sink); o += k; }
        sp.flush(sink);
        h.close_pending(); h.show();
        if (sp.refused() || h.refused) refused++;
        pictures += h.pictures; fields += h.fields; errors += h.errors; dropped += h.dropped; clamped += h.clamped; lone += h.lone; dual += h.n_dual; m16x8 += h.n_16x8;
    }
    printf("ok: %d trials, %ld pictures decoded (%ld field pictures), %ld errors, %ld refused, %ld dropped, %ld clamped macroblocks, %ld lone fields, "
           "%ld dual-prime and %ld 16x8 macroblocks\n", trials, pictures, fields, errors, refused, dropped, clamped, lone, dual, m16x8);
    return 0;
}
