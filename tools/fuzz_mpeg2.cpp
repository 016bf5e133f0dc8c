// tools/fuzz_mpeg2.cpp -- the MPEG-2 host path (Mpeg2Splitter, mpeg2_decode_picture, the reconstruction of mpeg2_recon.h with the anchor rules of
// INTEGRATION.md "MPEG-2") on mutated streams, built with AddressSanitizer / UBSan (host sanitizers; `make -C tools fuzz_mpeg2_asan`).  Nothing here
// touches a device.
//   fuzz_mpeg2_asan <stream.m2v> <seed> <trials>
// Trial 0 feeds the stream as it is; the others flip, insert, delete and truncate bytes and feed the result in random chunks.
#include "../jmcodec_amd/csrc/mpeg2_syntax.h"
#include "../jmcodec_amd/csrc/mpeg2_recon.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

using namespace jmamd;

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: fuzz_mpeg2_asan <stream> <seed> <trials>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> src; { uint8_t buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) src.insert(src.end(), buf, buf + k); }
    fclose(f);
    std::mt19937 rng((unsigned)atoi(argv[2]));
    const int trials = atoi(argv[3]);
    long pictures = 0, damaged = 0, refused = 0, dropped = 0, clamped = 0;
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
        Mpeg2Splitter sp; Mpeg2Jobs jobs;
        std::shared_ptr<std::vector<uint8_t>> anchor[2]; int aw = 0, ah = 0;
        auto sink = [&](Mpeg2Pic &pic) {
            const int mb_w = pic.seq.mb_w(), mb_h = pic.seq.mb_h();
            if (!pic.have_ext) { damaged++; return; }
            if (mb_w > 64 || mb_h > 64) return;                           // (a mutated size field: keep the trial short)
            if (mb_w != aw || mb_h != ah) { anchor[0].reset(); anchor[1].reset(); aw = mb_w; ah = mb_h; }
            if ((pic.type == 2 && !anchor[1]) || (pic.type == 3 && (!anchor[0] || !anchor[1]))) { dropped++; return; }
            bool refuse = false;
            if (!mpeg2_decode_picture(pic, jobs, &refuse).empty()) { if (refuse) { refused++; return; } damaged++; }
            clamped += jobs.clamped;
            const int W = mb_w * 16, H = mb_h * 16;
            auto cur = std::make_shared<std::vector<uint8_t>>((size_t)W * H * 3 / 2);       // exactly the surface: a read or store outside it is caught
            Mpeg2PicParams pp = {};
            pp.surf = cur->data(); pp.pitch = W; pp.chroma_offset = W * H; pp.mb_w = mb_w; pp.mb_h = mb_h;
            pp.ref[0] = pic.type == 2 ? anchor[1]->data() : (pic.type == 3 ? anchor[0]->data() : nullptr);
            pp.ref[1] = pic.type == 3 ? anchor[1]->data() : nullptr;
            pp.n_entries = (int)jobs.entries.size(); pp.dc_mult = 8 >> pic.intra_dc_precision;
            pp.mbs = jobs.mbs.data(); pp.entries = jobs.entries.data();
            memcpy(pp.w, pic.seq.w, sizeof pp.w);
            mpeg2_reconstruct_host(pp);
            if (pic.type != 3) { anchor[0] = anchor[1]; anchor[1] = cur; }
            pictures++;
        };
        for (size_t o = 0; o < d.size();) { const size_t k = std::min(d.size() - o, (size_t)(t % 3 == 0 ? d.size() : 1 + rng() % 300)); sp.feed(d.data() + o, k, sink); o += k; }
        sp.flush(sink);
        if (sp.refused()) refused++;
    }
    printf("ok: %d trials, %ld pictures decoded, %ld damaged, %ld refused, %ld dropped, %ld clamped macroblocks\n", trials, pictures, damaged, refused, dropped, clamped);
    return 0;
}
