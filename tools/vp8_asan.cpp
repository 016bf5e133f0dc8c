// tools/vp8_asan.cpp -- the lane routines of vp8_recon.h, which k_vp8_recon and k_vp8_filter run, walked on the CPU in the kernels' wavefront order
// over heap surfaces of EXACTLY the device's extent (16 mb_w x 16 mb_h luma samples + chroma, pitch = 16 mb_w), built with AddressSanitizer / UBSan
// (host sanitizers; `make -C tools vp8_asan`).  A read or a store outside a surface, the job list or a work area is caught.  Nothing here touches a device.
//   vp8_asan <seed> <trials>
// Every trial takes the sizes of the GPU tests (one macroblock; 3 x 2; cropped; one row of 17; 17 rows = a second band; a second band with live
// neighbours) with a random job list: valid ones (what vp8_validate_jobs accepts) and damaged ones -- modes, segments, levels, block numbers,
// first / count out of range, as no parser of ours writes them: the routines clamp what they index with.
#include "../jmcodec_amd/csrc/vp8_syntax.h"
#include "../jmcodec_amd/csrc/vp8_recon.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

using namespace jmamd;

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: vp8_asan <seed> <trials>\n"); return 2; }
    std::mt19937 rng((unsigned)atoi(argv[1]));
    const int trials = atoi(argv[2]);
    static const int sizes[][2] = {{16, 16}, {48, 32}, {53, 37}, {272, 16}, {16, 272}, {80, 272}};
    long pictures = 0, invalid = 0; unsigned long long sum = 0;
    for (int t = 0; t < trials; t++) for (auto &sz : sizes) {
        const int mb_w = (sz[0] + 15) / 16, mb_h = (sz[1] + 15) / 16, n = mb_w * mb_h;
        const bool damage = t % 2 == 1;
        // exact-size heap arrays: the sanitizer sees every access beyond them
        std::unique_ptr<Vp8Mb[]> mbs(new Vp8Mb[n]);
        std::vector<uint32_t> ent;
        for (int i = 0; i < n; i++) {
            Vp8Mb &m = mbs[i]; memset(&m, 0, sizeof m);
            m.ymode = (uint8_t)(rng() % 5); m.uvmode = (uint8_t)(rng() % 4); m.segment = (uint8_t)(rng() % 4); m.level = (uint8_t)(rng() % 64);
            for (auto &b : m.bmodes) b = (uint8_t)(rng() % 10);
            m.first = (uint32_t)ent.size();
            const int cnt = (int)(rng() % 3 == 0 ? 0 : rng() % 60);
            for (int e = 0; e < cnt; e++) {
                int blk = (int)(rng() % (m.ymode == VP8_B_PRED ? 24 : 25));
                const int lv = (int)(rng() % 4200) - 2100;
                ent.push_back((uint32_t)(rng() % 16) | (uint32_t)blk << 4 | (uint32_t)(uint16_t)(int16_t)lv << 16);
                m.nz |= 1u << blk;
            }
            m.count = (uint16_t)cnt;
            if (cnt || m.ymode == VP8_B_PRED) m.flags |= VP8_MB_INNER;
            if (damage && rng() % 3 == 0) switch (rng() % 6) {
                case 0: m.ymode = (uint8_t)rng(); break;
                case 1: m.uvmode = (uint8_t)rng(); m.segment = (uint8_t)rng(); break;
                case 2: m.level = (uint8_t)rng(); m.flags = (uint8_t)rng(); break;
                case 3: m.first = (uint32_t)rng(); break;
                case 4: m.count = (uint16_t)rng(); m.nz = (uint32_t)rng(); break;
                default: for (auto &b : m.bmodes) b = (uint8_t)rng(); break;
            }
        }
        if (damage) for (auto &e : ent) if (rng() % 8 == 0) e = (uint32_t)rng();
        std::unique_ptr<uint32_t[]> entries(new uint32_t[ent.size() ? ent.size() : 1]);
        if (!ent.empty()) memcpy(entries.get(), ent.data(), ent.size() * 4);
        const int W = mb_w * 16, Hh = mb_h * 16;
        std::unique_ptr<uint8_t[]> surf(new uint8_t[(size_t)W * Hh * 3 / 2]);
        memset(surf.get(), 128, (size_t)W * Hh * 3 / 2);
        Vp8PicParams pp = {};
        pp.surf = surf.get(); pp.pitch = W; pp.chroma_offset = W * Hh; pp.mb_w = mb_w; pp.mb_h = mb_h;
        pp.n_entries = (int)ent.size(); pp.filter_type = (int)(rng() % 2); pp.sharpness = (int)(rng() % 8); pp.filtered = 1;
        pp.mbs = mbs.get(); pp.entries = entries.get();
        for (auto &s : pp.dq) for (auto &q : s) q = (int16_t)(4 + rng() % 437);
        if (!damage) {
            Vp8Pic pic; pic.mb_w = mb_w; pic.mb_h = mb_h; pic.mbs.assign(mbs.get(), mbs.get() + n); pic.entries = ent;
            if (!vp8_validate_jobs(pic).empty()) { fprintf(stderr, "a valid list was not accepted: %s\n", vp8_validate_jobs(pic).c_str()); return 1; }
        } else {
            Vp8Pic pic; pic.mb_w = mb_w; pic.mb_h = mb_h; pic.mbs.assign(mbs.get(), mbs.get() + n); pic.entries = ent;
            if (!vp8_validate_jobs(pic).empty()) invalid++;
        }
        vp8_reconstruct_host(pp);
        vp8_filter_host(pp);
        for (size_t i = 0; i < (size_t)W * Hh * 3 / 2; i += 97) sum += surf[i];
        pictures++;
    }
    printf("ok: %d trials, %ld pictures reconstructed and filtered, %ld damaged lists the validation refuses, checksum %llu\n", trials, pictures, invalid, sum);
    return 0;
}
