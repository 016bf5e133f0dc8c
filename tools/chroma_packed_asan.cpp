// tools/chroma_packed_asan.cpp -- the lane routines of k_rgb_pack444 (jmcodec_amd/csrc/chroma_packed.h; INTEGRATION.md "RGB output": interpolated
// chroma) walked on the CPU over a fixed handful of geometries, built with AddressSanitizer / UBSan (host sanitizers; `make -C tools
// chroma_packed_asan`).  Source, destination AND the six tap tables are heap buffers of exactly their size: a read outside the surface, a write outside
// the frame or a table index outside its axis aborts.  Nothing here touches a device.
#include "../tests/native/chroma_packed_walk.h"
#include <cstdio>
#include <memory>

using namespace jmamd;

struct Geo { int W, H, cx, cy, cw, ch, tw, th, rx, ry, rw, rh, lone; };      // rw == 0: no placement
static const Geo kGeos[] = {
    {70, 22, 0, 0, 70, 22, 70, 22, 0, 0, 0, 0, 0},            // identity geometry, no multiple of 64 / 16
    {70, 22, 2, 2, 66, 18, 50, 26, 0, 0, 0, 0, 0},            // odd chroma origin, down and up
    {2, 2, 0, 0, 2, 2, 2, 2, 0, 0, 0, 0, 0},                  // Sc = 1
    {2, 2, 0, 0, 2, 2, 8, 8, 0, 0, 0, 0, 0},                  // ... 1:4 up
    {16, 10, 0, 0, 16, 10, 64, 40, 0, 0, 0, 0, 0},            // 1:4 up
    {480, 272, 0, 0, 480, 272, 60, 34, 0, 0, 0, 0, 0},        // 8:1 down
    {130, 34, 0, 0, 130, 34, 130, 34, 0, 0, 0, 0, 2},         // a lone bottom field with H % 4 == 2
    {120, 68, 0, 0, 120, 68, 96, 48, 2, 2, 60, 34, 0},        // placed: rx % 4 == 2
    {100, 40, 0, 0, 100, 40, 128, 48, 40, 8, 50, 20, 1},      // ... crosses column 64 and row 16, top field alone
    {64, 32, 0, 0, 64, 32, 160, 64, 128, 48, 32, 16, 0},      // ... most tiles fill only
    {90, 70, 0, 0, 90, 70, 96, 80, 4, 6, 90, 70, 0},          // ... pure padding
    {8, 8, 0, 0, 8, 8, 32, 16, 10, 6, 2, 2, 0},               // ... the smallest rectangle
};

int main() {
    int walks = 0;
    for (const Geo &g : kGeos) {
        const int pitch = g.W;                                                      // tight rows
        const int hs = g.H + (g.lone && g.H % 4 ? 2 : 0);                            // a lone field of H % 4 == 2 reads the next chroma row
        const size_t src_n = (size_t)pitch * hs * 3 / 2;
        std::unique_ptr<uint8_t[]> src(new uint8_t[src_n]);
        for (size_t i = 0; i < src_n; i++) src[i] = (uint8_t)(i * 131 + (i >> 8) * 17);
        const int rect[4] = {g.rx, g.ry, g.rw, g.rh};
        for (int loc = 0; loc < 6; loc++)
            for (int dtype = RGB_U8; dtype <= RGB_BF16; dtype++) {
                const int planar = (loc + dtype) & 1, mis = loc & 1;                 // mis: the frame starts one sample behind the allocation's start
                const int sz = dtype == RGB_U8 ? 1 : (dtype == RGB_F32 ? 4 : 2);
                const size_t n = (size_t)3 * g.tw * g.th * sz;
                std::unique_ptr<uint8_t[]> dst(new uint8_t[n + (mis ? sz : 0)]);
                RgbJob rj = {};
                rj.s = ScaleJob{src.get(), dst.get() + (mis ? sz : 0), pitch, pitch * hs, g.cx, g.cy, g.tw, g.th, 0, g.lone, {}};
                walk::Tables tables; walk::ChromaTables ctables;
                if (!walk::place(rj.s, tables, g.cw, g.ch, rect, 0) ||
                    !ctables.build(g.cw, g.ch, rj.s.rw ? rj.s.rw : g.tw, rj.s.rw ? rj.s.rh : g.th, loc, rj.cax)) {
                    fprintf(stderr, "%dx%d -> %dx%d: no tap tables\n", g.cw, g.ch, g.tw, g.th); return 1; }
                rj.chroma = 1;
                rj.cy = 19077; rj.crv = 29372; rj.cgu = 3494; rj.cgv = 8731; rj.cbu = 34610; rj.yo = 16;      // BT.709, limited range
                rj.dtype = dtype; rj.planar = planar; rj.bgr = mis; rj.fill = 0x123456;
                for (int k = 0; k < 3; k++) { rj.k[k] = (1.0f / 255.0f) * (1.0f / 16384.0f); rj.b[k] = -0.5f; }
                if (!walk::chroma_rgb_frame(rj)) { fprintf(stderr, "%dx%d -> %dx%d: row guard\n", g.cw, g.ch, g.tw, g.th); return 1; }
                walks++;
            }
    }
    printf("ok: %d walks over %d geometries\n", walks, (int)(sizeof kGeos / sizeof kGeos[0]));
    return 0;
}
