// tools/mpeg2_vlc_asan.cpp -- option mpeg2_device_vlc under AddressSanitizer / UBSan (host sanitizers; `make -C tools mpeg2_vlc_asan`): the prescan and
// the device routine of k_mpeg2_vlc walked on the CPU over heap buffers of exactly the sizes the device gets (tests/native/mpeg2_vlc_walk.h).  A
// stand-alone program; nothing here touches a device.
//   mpeg2_vlc_asan <stream.m2v> <seed> <trials> [<seconds>]
// Trial 0 walks the stream as it is and requires that every picture the prescan accepts agrees with the host decoder.  The others flip bits,
// overwrite bytes, truncate, and duplicate and swap slices, and require the bounds: iterations, capacity, entry ranges, spans that tile the
// picture -- and, wherever the host decoder and the walk both call a picture clean, equal records and entries.  Stops early after <seconds>
// (default 60).
#include "../tests/native/mpeg2_vlc_walk.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <random>

using namespace jmamd;

// the slice units (start codes 01..AF) of d: [begin, end) each
static std::vector<std::pair<size_t, size_t>> slice_units(const std::vector<uint8_t> &d) {
    std::vector<size_t> sc;
    for (size_t i = 0; i + 4 <= d.size(); i++) if (d[i] == 0 && d[i + 1] == 0 && d[i + 2] == 1) sc.push_back(i);
    std::vector<std::pair<size_t, size_t>> out;
    for (size_t k = 0; k < sc.size(); k++) {
        const int code = d[sc[k] + 3];
        if (code >= 0x01 && code <= 0xAF) out.push_back({sc[k], k + 1 < sc.size() ? sc[k + 1] : d.size()});
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: mpeg2_vlc_asan <stream> <seed> <trials> [<seconds>]\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> src; { uint8_t buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) src.insert(src.end(), buf, buf + k); }
    fclose(f);
    std::mt19937 rng((unsigned)atoi(argv[2]));
    const int trials = atoi(argv[3]);
    const double seconds = argc > 4 ? atof(argv[4]) : 60.0;
    const auto t0 = std::chrono::steady_clock::now();
    long pictures = 0, accepted = 0, damaged_slices = 0, slices = 0, compared = 0;
    int done = 0;
    for (int t = 0; t < trials; t++, done++) {
        if (t > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) break;
        std::vector<uint8_t> d = src;
        if (t > 0 && !d.empty()) {
            const int n_mut = 1 + (int)(rng() % 5);
            for (int m = 0; m < n_mut && !d.empty(); m++) {
                const size_t at = rng() % d.size();
                switch (rng() % 6) {
                case 0: case 1: d[at] ^= (uint8_t)(1u << (rng() % 8)); break;
                case 2: d[at] = (uint8_t)rng(); break;
                case 3: if (rng() % 3 == 0) d.resize(at); break;
                case 4: { auto u = slice_units(d); if (u.empty()) break;                       // a slice twice
                    const auto s = u[rng() % u.size()]; std::vector<uint8_t> c(d.begin() + (long)s.first, d.begin() + (long)s.second);
                    d.insert(d.begin() + (long)s.second, c.begin(), c.end()); break; }
                default: { auto u = slice_units(d); if (u.size() < 2) break;                   // two neighbouring slices swapped
                    const size_t k = rng() % (u.size() - 1); if (u[k].second != u[k + 1].first) break;
                    std::rotate(d.begin() + (long)u[k].first, d.begin() + (long)u[k].second, d.begin() + (long)u[k + 1].second); break; }
                }
            }
        }
        Mpeg2Splitter sp; Mpeg2Jobs jobs; Mpeg2VlcWalk w;
        bool bad = false;
        auto sink = [&](Mpeg2Pic &pic) {
            if (!pic.have_ext) return;
            if (pic.seq.mb_w() * pic.seq.mb_h() > 4096) return;             // (a mutated size field: keep the trial short)
            bool refuse = false;
            const std::string e = mpeg2_decode_picture(pic, jobs, &refuse);
            mpeg2_vlc_walk(pic, w);
            pictures++;
            if (!w.reject.empty()) return;
            accepted++; slices += (long)w.slices.size(); damaged_slices += w.damaged;
            if (!w.bound_ok || !w.tiled) { fprintf(stderr, "trial %d: a bound was broken (iterations / capacity / spans)\n", t); bad = true; }
            if (refuse != w.dual_prime && e.empty()) { fprintf(stderr, "trial %d: the dual-prime status differs\n", t); bad = true; }
            const bool both_clean = e.empty() && !w.error();
            if ((t == 0 || both_clean) && !refuse && !w.dual_prime) {
                compared++;
                if (mpeg2_vlc_compare(w, jobs) != 0 || (t == 0 && (w.error() != !e.empty() || w.clamped != jobs.clamped))) {
                    fprintf(stderr, "trial %d: the walk differs from the host decoder\n", t); bad = true; }
            }
        };
        sp.feed(d.data(), d.size(), sink);
        sp.flush(sink);
        if (bad) return 1;
    }
    if (done < trials) printf("(stopped after %d of %d trials: %.0f s)\n", done, trials, seconds);
    printf("ok: %d trials, %ld pictures, %ld walked, %ld compared, %ld slices, %ld damaged\n", done < trials ? done : trials, pictures, accepted, compared, slices, damaged_slices);
    return 0;
}
