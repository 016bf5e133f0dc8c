// tools/md5_asan.cpp -- the lane routines of k_hevc_md5 (jmcodec_amd/csrc/md5_packed.h) playing the kernel on the CPU, built with AddressSanitizer /
// UBSan (host sanitizers; `make -C tools md5_asan`).  Every surface is a heap buffer of exactly the bytes the hash covers -- the last chroma row ends
// with the allocation -- so a read past a row's samples aborts.  Nothing here touches a device, and nothing here is the expected value's source except
// the RFC 1321 test suite: tests/test_md5_host.py compares the printed digests with hashlib.
//   md5_asan                                       prints "tile <kMd5TileBytes>", runs the RFC's test suite and a few exact-size walks, prints "ok: ..."
//   md5_asan raw FILE                              the file's bytes as one stream through the padding and block routines; prints the digest
//   md5_asan surface FILE pitch chroma_offset w h  the file is an NV12 surface: the kernel's every tile and staging item in order; prints three digests
#include "../jmcodec_amd/csrc/md5_packed.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace jmamd;

static std::string hex(const uint32_t *state) {
    char s[33];
    for (int k = 0; k < 16; k++) snprintf(s + 2 * k, 3, "%02x", (state[k >> 2] >> (8 * (k & 3))) & 255u);
    return s;
}

// k_hevc_md5 for one component, lane by lane: a loop over lanes stands for the lanes of a workgroup, the end of a loop nest for its barrier.  Wave 0
// (lanes 0..63, every one the same chain: lane 0 is played) walks tile t while lanes 64..255 stage tile t + 1 into the other half of the buffer.
static std::string play_kernel(const uint8_t *surf, int pitch, int chroma_offset, int w, int h, int c, bool wide) {
    static uint32_t tile[2][md5::kTileWords];
    const uint32_t n = md5::comp_bytes(w, h, c);
    const int tiles = md5::tile_count(n);
    auto stage = [&](int t, int first, int step) {
        for (int i = first; i < md5::tile_items(n, t); i += step) md5::stage_item(surf, pitch, chroma_offset, w, h, c, t, i, wide, &tile[t & 1][4 * i]);
    };
    for (int tid = 0; tid < 256; tid++) stage(0, tid, 256);
    uint32_t state[4] = {md5::kInit[0], md5::kInit[1], md5::kInit[2], md5::kInit[3]};
    for (int t = 0; t < tiles; t++) {
        for (int tid = 64; tid < 256; tid++) if (t + 1 < tiles) stage(t + 1, tid - 64, 192);
        for (int b = 0; b < md5::tile_blocks(n, t); b++) md5::block(state, &tile[t & 1][16 * b]);
    }
    return hex(state);
}

// a stream of n bytes that is no picture: a surface of width n + (n & 1) would change the length, so the bytes go through pad_byte and block directly
static std::string md5_raw(const std::vector<uint8_t> &data) {
    const uint32_t n = (uint32_t)data.size();
    uint32_t state[4] = {md5::kInit[0], md5::kInit[1], md5::kInit[2], md5::kInit[3]};
    for (uint32_t q = 0; q < md5::padded_bytes(n); q += 64) {
        uint32_t m[16] = {};
        for (uint32_t j = 0; j < 64; j++) m[j >> 2] |= (q + j < n ? (uint32_t)data[q + j] : md5::pad_byte(q + j, n)) << (8 * (j & 3));
        md5::block(state, m);
    }
    return hex(state);
}

static bool read_all(const char *path, std::vector<uint8_t> &v) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return true;
}

static int fail(const char *what, long a = 0, long b = 0) { fprintf(stderr, "FAILED: %s (%ld, %ld)\n", what, a, b); return 1; }

// an exact-size surface of pseudo-random bytes: both load paths must agree with the stream taken out byte by byte
static int walk(int w, int h, int pitch, unsigned seed, int &walks) {
    const int chroma_offset = pitch * h;
    const size_t bytes = (size_t)chroma_offset + (size_t)pitch * (h / 2 - 1) + w;
    std::unique_ptr<uint8_t[]> surf(new uint8_t[bytes]);
    unsigned s = seed;
    for (size_t i = 0; i < bytes; i++) { s = s * 1664525u + 1013904223u; surf[i] = (uint8_t)(s >> 24); }
    for (int c = 0; c < 3; c++) {
        std::vector<uint8_t> plain(md5::comp_bytes(w, h, c));
        for (uint32_t q = 0; q < plain.size(); q++) plain[q] = surf[md5::sample_offset(c, q, w, pitch, chroma_offset)];
        const std::string want = md5_raw(plain);
        for (int wide = 0; wide < 2; wide++) {
            if (wide && ((((uintptr_t)surf.get()) | (uintptr_t)pitch | (uintptr_t)chroma_offset) & 15)) continue;
            if (play_kernel(surf.get(), pitch, chroma_offset, w, h, c, wide != 0) != want) return fail("a surface's component", w, h);
            walks++;
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "raw")) {
        std::vector<uint8_t> data;
        if (!read_all(argv[2], data)) return fail("cannot read the file");
        printf("%s\n", md5_raw(data).c_str());
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "surface")) {
        std::vector<uint8_t> data;
        if (!read_all(argv[2], data)) return fail("cannot read the file");
        const int pitch = atoi(argv[3]), chroma_offset = atoi(argv[4]), w = atoi(argv[5]), h = atoi(argv[6]);
        if (w < 2 || h < 2 || ((w | h) & 1) || pitch < w || chroma_offset < 0) return fail("arguments");
        if (data.size() < (size_t)chroma_offset + (size_t)pitch * (h / 2 - 1) + w || data.size() < (size_t)pitch * (h - 1) + w) return fail("the file is too short");
        // the exact size, on the heap: whatever the routines read beyond the file's bytes is a report
        std::unique_ptr<uint8_t[]> surf(new uint8_t[data.size()]);
        memcpy(surf.get(), data.data(), data.size());
        const bool wide = ((((uintptr_t)surf.get()) | (uintptr_t)pitch | (uintptr_t)chroma_offset) & 15) == 0;
        for (int c = 0; c < 3; c++) {
            const std::string d = play_kernel(surf.get(), pitch, chroma_offset, w, h, c, wide);
            if (wide && play_kernel(surf.get(), pitch, chroma_offset, w, h, c, false) != d) return fail("the two load paths differ", c);
            printf("%s\n", d.c_str());
        }
        return 0;
    }
    if (argc != 1) { fprintf(stderr, "usage: %s [raw FILE | surface FILE pitch chroma_offset w h]\n", argv[0]); return 2; }
    printf("tile %d\n", md5::kMd5TileBytes);
    // RFC 1321, appendix A.5
    static const char *const suite[][2] = {
        {"", "d41d8cd98f00b204e9800998ecf8427e"},
        {"a", "0cc175b9c0f1b6a831c399e269772661"},
        {"abc", "900150983cd24fb0d6963f7d28e17f72"},
        {"message digest", "f96b697d7cb7938d525a2f31aaf161d0"},
        {"abcdefghijklmnopqrstuvwxyz", "c3fcd3d76192e4007dfb496cca67e13b"},
        {"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", "d174ab98d277d9f5a5611c2c9f419d9f"},
        {"12345678901234567890123456789012345678901234567890123456789012345678901234567890", "57edf4a22be3c955ac49da2e2107b67a"}};
    for (auto &t : suite) {
        const std::vector<uint8_t> v(t[0], t[0] + strlen(t[0]));
        if (md5_raw(v) != t[1]) return fail("RFC 1321 test suite", (long)v.size());
    }
    // the kernel's walk over a surface holding the suite's 62-byte string twice as its luma (2 x 62): the same staging and tiling as a picture's
    {
        const char *t = suite[5][0];
        std::unique_ptr<uint8_t[]> surf(new uint8_t[2 * 62 + 62]);
        memcpy(surf.get(), t, 62); memcpy(surf.get() + 62, t, 62); memset(surf.get() + 124, 0, 62);
        std::vector<uint8_t> twice(t, t + 62); twice.insert(twice.end(), t, t + 62);
        if (play_kernel(surf.get(), 62, 124, 62, 2, 0, false) != md5_raw(twice)) return fail("the suite's string as a surface");
    }
    // exact-size walks: what lies around the block (64), the 16-byte run and the tile, tight and padded
    const int T = md5::kMd5TileBytes;
    const int kSizes[][2] = {{2, 2}, {8, 8}, {6, 10}, {14, 4}, {10, 22}, {14, 16}, {14, 18}, {16, 16}, {24, 16}, {66, 34}, {6, (T - 4) / 6}, {64, T / 64},
                             {64, T / 64 + 2}, {96, 80}, {176, 144}, {200, 120}, {520, 40}};
    int walks = 0;
    for (auto &sz : kSizes) for (int pad : {0, 16, 6})
        if (walk(sz[0], sz[1], (pad == 16 ? (sz[0] + 15) / 16 * 16 : sz[0]) + pad, 4321u + (unsigned)sz[0] * 31u + (unsigned)pad, walks)) return 1;
    printf("ok: %d walks over %d sizes\n", walks, (int)(sizeof kSizes / sizeof kSizes[0]));
    return 0;
}
