// tools/deblock_packed_asan.cpp -- the H.264 edge filters of the deblocking kernels (jmcodec_amd/csrc/deblock_packed.h) run on the CPU, built with
// AddressSanitizer / UBSan (host sanitizers; `make -C tools deblock_packed_asan`).  Lines, parameters and results live in heap buffers of exactly the
// bytes the routines cover, so an access past a line aborts; the packed, branch-free and scalar forms are compared with the literal restatement of
// 8.7.2.2 - 8.7.2.4 in tests/native/deblock_packed_check.cpp over bS 0..4.  alpha / beta / tC0 are not looked up here (tests/test_deblock_packed.py walks
// Tables 8-16 / 8-17): they are drawn from everything a table could hold, 0..255 / 0..18 / 0..25, by a fixed linear congruential generator.  Built as C++20, where shifting a negative value left is defined (the filters shift differences, as
// the device code does).  Nothing here touches a device.  Prints "ok: ..." and returns 0.
#include "../tests/native/deblock_packed_check.cpp"
#include <cstdio>
#include <cstring>
#include <memory>

int main() {
    unsigned s = 0x4A4D0871u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    long lines = 0, filtered = 0;
    for (int round = 0; round < 4000; round++) {
        const int n = 1 + (int)(rnd() % 97);
        std::unique_ptr<uint8_t[]> in(new uint8_t[8 * n]), in4(new uint8_t[4 * n]), bS(new uint8_t[n]), al(new uint8_t[n]), be(new uint8_t[n]), tc(new uint8_t[3 * n]);
        std::unique_ptr<uint8_t[]> want(new uint8_t[8 * n]), a(new uint8_t[8 * n]), b(new uint8_t[8 * n]), want4(new uint8_t[4 * n]), a4(new uint8_t[4 * n]), b4(new uint8_t[4 * n]);
        for (int i = 0; i < n; i++) {
            bS[i] = (uint8_t)(rnd() % 5); al[i] = (uint8_t)(rnd() % 256); be[i] = (uint8_t)(rnd() % 19);
            for (int k = 0; k < 3; k++) tc[3 * i + k] = (uint8_t)(rnd() % 26);
            const int level = (int)(rnd() % 256), amp = 1 + (int)(rnd() % (round % 3 == 0 ? 128 : 10));
            for (int k = 0; k < 8; k++) { int v = level + (int)(rnd() % (2 * amp + 1)) - amp; in[8 * i + k] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
            for (int k = 0; k < 4; k++) in4[4 * i + k] = in[8 * i + 2 + k];
        }
        uint64_t cl[L_COUNT] = {0}, cc[C_COUNT] = {0};
        dbp_luma_literal(n, in.get(), bS.get(), al.get(), be.get(), tc.get(), want.get(), cl);
        dbp_luma_packed(n, in.get(), bS.get(), al.get(), be.get(), tc.get(), a.get());
        dbp_luma_scalar(n, in.get(), bS.get(), al.get(), be.get(), tc.get(), b.get());
        dbp_chroma_literal(n, in4.get(), bS.get(), al.get(), be.get(), tc.get(), want4.get(), cc);
        dbp_chroma_packed(n, in4.get(), bS.get(), al.get(), be.get(), tc.get(), a4.get());
        dbp_chroma_scalar(n, in4.get(), bS.get(), al.get(), be.get(), tc.get(), b4.get());
        if (memcmp(want.get(), a.get(), 8 * n) || memcmp(want.get(), b.get(), 8 * n) || memcmp(want4.get(), a4.get(), 4 * n) || memcmp(want4.get(), b4.get(), 4 * n) ||
            dbp_luma_packed_out_of_range(n, in.get(), bS.get(), al.get(), be.get(), tc.get())) { fprintf(stderr, "FAILED: round %d\n", round); return 1; }
        lines += n; filtered += (long)(cl[L_ON_BS1] + cl[L_ON_BS2] + cl[L_ON_BS3] + cl[L_ON_BS4]);
    }
    printf("ok: %ld lines (%ld filtered), four forms equal the clause\n", lines, filtered);
    return 0;
}
