// tools/jpeg_entropy_asan.cpp -- option jpeg_device_entropy under AddressSanitizer / UBSan (host sanitizers; `make -C tools jpeg_entropy_asan`): the
// segmenter and the device routine of k_jpeg_entropy walked on the CPU over heap buffers of exactly the sizes the device gets
// (tests/native/jpeg_entropy_walk.h).  A stand-alone program; nothing here touches a device.
//   jpeg_entropy_asan <stream.mjpeg> <seed> <trials> [<seconds> [damaged]]
// Trial 0 walks the stream as it is and requires that every picture agrees with the host decoder (and, unless "damaged" is given, that none is
// damaged); the others flip, insert, delete and truncate
// bytes -- mostly inside the entropy-coded data -- and require the bounds: iterations, capacity, every block in exactly one segment, undamaged
// segments equal to the host decoder's blocks wherever the host decoder got as far.  Stops early after <seconds> (default 20).
#include "../tests/native/jpeg_entropy_walk.h"
#include <chrono>
#include <cstdio>
#include <random>

using namespace jmamd;

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: jpeg_entropy_asan <stream> <seed> <trials> [<seconds>]\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> src; { uint8_t buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) src.insert(src.end(), buf, buf + k); }
    fclose(f);
    std::mt19937 rng((unsigned)atoi(argv[2]));
    const int trials = atoi(argv[3]);
    const double seconds = argc > 4 ? atof(argv[4]) : 20.0;
    const bool expect_clean = !(argc > 5 && std::string(argv[5]) == "damaged");
    const auto t0 = std::chrono::steady_clock::now();
    long pictures = 0, damaged_segments = 0, segments = 0, complaints = 0;
    int done = 0;
    for (int t = 0; t < trials; t++, done++) {
        if (t > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) break;
        std::vector<uint8_t> d = src;
        if (t > 0 && !d.empty()) {
            const int n_mut = 1 + (int)(rng() % 6);
            for (int m = 0; m < n_mut && !d.empty(); m++) {
                const size_t at = rng() % d.size();
                switch (rng() % 6) {
                case 0: d[at] ^= (uint8_t)(1u << (rng() % 8)); break;
                case 1: d[at] = (uint8_t)rng(); break;
                case 2: d.insert(d.begin() + (long)at, (uint8_t)(rng() % 2 ? 0xFF : rng())); break;
                case 3: d.erase(d.begin() + (long)at); break;
                case 4: { const uint8_t mk[2] = {0xFF, (uint8_t)(0xD0 + rng() % 8)}; d.insert(d.begin() + (long)at, mk, mk + 2); break; }      // a surplus RSTn
                default: if (rng() % 4 == 0) d.resize(at); break;
                }
            }
        }
        JpegSplitter sp; JpegTables tab; JpegJobs jobs; JpegEntropyWalk w;
        bool bad = false;
        auto sink = [&](const uint8_t *p, size_t len, bool) {
            JpegPic pic; bool refuse = false;
            if (!jpeg_parse_picture(p, len, tab, pic, &refuse).empty()) return;
            if (pic.width > 1024 || pic.height > 1024) return;           // (a mutated size field: keep the trial short)
            jpeg_entropy_walk(pic, p, len, w);
            const bool host_ok = jpeg_decode_scan(pic, p, len, jobs).empty();
            pictures++; segments += (long)w.segs.size(); damaged_segments += w.damaged; complaints += !w.seg_error.empty();
            if (!w.bound_ok || !w.covered) { fprintf(stderr, "trial %d: a bound was broken (iterations / capacity / coverage)\n", t); bad = true; }
            // a picture the host decoder accepts whole and the segmenter did not complain about: identical lists, no damage
            if (host_ok && w.seg_error.empty() && (w.damaged || jpeg_entropy_compare(pic, w, jobs))) {
                fprintf(stderr, "trial %d: the walk differs from the host decoder on a picture both accept\n", t); bad = true; }
            if (t == 0 && expect_clean && (!host_ok || w.damaged)) { fprintf(stderr, "the unmutated stream is damaged\n"); bad = true; }
        };
        sp.feed(d.data(), d.size(), sink);
        sp.flush(sink);
        if (bad) return 1;
    }
    if (done < trials) printf("(stopped after %d of %d trials: %.0f s)\n", done, trials, seconds);
    printf("ok: %d trials, %ld pictures walked, %ld segments, %ld damaged, %ld segmenter complaints\n", done < trials ? done : trials, pictures, segments,
           damaged_segments, complaints);
    return 0;
}
