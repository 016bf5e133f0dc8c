// tools/deint3_asan.cpp -- the strip routine of k_deint3 (jmcodec_amd/csrc/deint3_packed.h) under AddressSanitizer and UBSan: every work item of
// frames whose buffers are heap blocks of EXACTLY the bytes the surfaces hold, so a read or write one byte outside a plane is reported.  Sizes that
// are no multiple of 16, odd chroma row counts, pitches equal to the width and aligned ones (the 16-byte path), both kept fields, one output and
// two, NV12 and I420 destinations.  `deint3_asan overread` reads ONE byte behind such a block on purpose and must be stopped by the sanitizer: it shows
// that the blocks are guarded from their last byte on.  make -C tools deint3_asan && tools/deint3_asan   (tests/test_deint3_host.py runs both)
#include "../jmcodec_amd/csrc/deint3_packed.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace jmamd::dei;

// n bytes at a 16-byte boundary (the fast path needs 16-byte rows).  posix_memalign takes any size, so the allocation is n bytes and no more: the
// sanitizer's redzone starts at byte n
static uint8_t *block(size_t n, unsigned &seed) {
    void *v = nullptr;
    if (posix_memalign(&v, 16, n) != 0 || !v) abort();
    uint8_t *p = (uint8_t *)v;
    for (size_t i = 0; i < n; i++) { seed = seed * 1664525u + 1013904223u; p[i] = (uint8_t)(seed >> 24); }
    return p;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "overread")) {          // 162 bytes: 2 past a multiple of 16, like the last chroma row of a ragged plane
        unsigned s = 1u;
        volatile uint8_t *p = block(162, s);
        const uint8_t v = p[162];                            // the sanitizer ends the program here
        printf("deint3_asan: a read one byte behind a block went unnoticed (%u)\n", v);
        return 0;
    }
    static const int sizes[][2] = {{2, 4}, {16, 4}, {18, 6}, {30, 10}, {32, 16}, {34, 22}, {48, 18}, {90, 70}, {130, 70}, {176, 160}};
    unsigned seed = 12345u, frames = 0;
    for (auto &s : sizes) for (int aligned = 0; aligned < 2; aligned++) for (int fmt = 0; fmt < 2; fmt++) for (int parity = 0; parity < 2; parity++)
        for (int both = 0; both < 2; both++) {
            const int w = s[0], h = s[1];
            const int pitch = aligned ? (w + 15) & ~15 : w, qpitch = aligned ? ((w + 15) & ~15) + 16 : w, dp = fmt ? w : (aligned ? (w + 15) & ~15 : w);
            // the last row of a surface ends with its w bytes: the block is exact to the byte
            const size_t sn = (size_t)pitch * h + (size_t)pitch * (h / 2 - 1) + w, qn = (size_t)qpitch * h + (size_t)qpitch * (h / 2 - 1) + w;
            const size_t dn = fmt ? (size_t)w * h * 3 / 2 : (size_t)dp * h + (size_t)dp * (h / 2 - 1) + w;
            uint8_t *src = block(sn, seed), *prev = block(qn, seed), *d0 = block(dn, seed), *d1 = both ? block(dn, seed) : nullptr;
            for (size_t i = 0; i < sn && i < qn; i += 3) prev[i] = src[i];          // (some samples equal: both branches)
            for (int i = 0; i < frame2_items(w, h); i++)
                deint3_item(src, prev, d0, d1, pitch, pitch * h, qpitch, qpitch * h, w, h, dp, dp * h, fmt, parity, 1 + (int)(seed % 255u), i);
            free(src); free(prev); free(d0); free(d1);
            frames++;
        }
    printf("deint3_asan: %u frames ok\n", frames);
    return 0;
}
