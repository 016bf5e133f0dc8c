// tools/place_packed_asan.cpp -- the placed paths of the lane routines of k_scale_pack and k_rgb_pack (jmcodec_amd/csrc/scale_packed.h, rgb_packed.h;
// INTEGRATION.md "Placed output") walked on the CPU over a fixed handful of placements, built with AddressSanitizer / UBSan (host sanitizers;
// `make -C tools place_packed_asan`).  Source, destination AND the four tap tables are heap buffers of exactly their size: a read outside the surface,
// a write outside the frame or a table index outside [0, rw) / [0, rh) aborts.  Nothing here touches a device.
#include "../tests/native/place_packed_walk.h"
#include <cstdio>
#include <memory>

using namespace jmamd;

struct Geo { int W, H, cx, cy, cw, ch, tw, th, rx, ry, rw, rh, lone; };
static const Geo kGeos[] = {
    {120, 68, 0, 0, 120, 68, 96, 48, 2, 2, 60, 34, 0},        // rx % 4 == 2, the chroma origin is odd
    {8, 8, 0, 0, 8, 8, 32, 16, 10, 6, 2, 2, 0},               // the smallest rectangle
    {2, 2, 0, 0, 2, 2, 2, 4, 0, 2, 2, 2, 0},                  // ... in the smallest target that places it
    {40, 20, 0, 0, 40, 20, 128, 32, 70, 18, 20, 10, 1},       // inside one tile, top field alone
    {100, 40, 0, 0, 100, 40, 128, 48, 40, 8, 50, 20, 0},      // crosses column 64 and row 16
    {64, 32, 0, 0, 64, 32, 160, 64, 128, 48, 32, 16, 0},      // most tiles are fill only; the rectangle ends at the target's corner
    {90, 70, 2, 4, 80, 60, 70, 38, 6, 2, 58, 34, 2},          // target sizes that are no multiple of 4, bottom field alone
    {90, 70, 0, 0, 90, 70, 96, 80, 4, 6, 90, 70, 0},          // pure padding: k_rgb_pack<false>
    {130, 34, 0, 0, 130, 34, 134, 40, 2, 6, 130, 34, 2},      // ... of a lone bottom field with H % 4 == 2
    {480, 272, 0, 0, 480, 272, 96, 48, 18, 6, 60, 34, 0},     // 8:1 down into the rectangle
    {16, 10, 0, 0, 16, 10, 96, 48, 16, 4, 64, 40, 0},         // 1:4 up into the rectangle
    {60, 44, 4, 2, 52, 40, 98, 50, 46, 14, 52, 36, 0},        // the rectangle ends at the target's right / bottom edge
};

int main() {
    int walks = 0;
    for (const Geo &g : kGeos) {
        const int pitch = g.W;                                                      // tight rows: nothing behind a row's last sample but the next row
        const int hs = g.H + (g.lone && g.H % 4 ? 2 : 0);                            // surface rows: a lone field of H % 4 == 2 reads the next chroma row
        const size_t src_n = (size_t)pitch * hs * 3 / 2;
        std::unique_ptr<uint8_t[]> src(new uint8_t[src_n]);
        for (size_t i = 0; i < src_n; i++) src[i] = (uint8_t)(i * 131 + (i >> 8) * 17);
        const int rect[4] = {g.rx, g.ry, g.rw, g.rh};
        walk::Tables tables;
        ScaleJob sj{src.get(), nullptr, pitch, pitch * hs, g.cx, g.cy, g.tw, g.th, 0, g.lone, {}};
        if (!walk::place(sj, tables, g.cw, g.ch, rect, 0x123456)) { fprintf(stderr, "%dx%d -> %dx%d: no tap tables\n", g.cw, g.ch, g.rw, g.rh); return 1; }
        for (int fmt = 0; fmt < 2; fmt++) {
            std::unique_ptr<uint8_t[]> dst(new uint8_t[(size_t)g.tw * g.th * 3 / 2]);
            sj.dst = dst.get(); sj.out_fmt = fmt;
            if (!walk::placed_scale_frame(sj)) { fprintf(stderr, "%dx%d -> %dx%d: row guard\n", g.cw, g.ch, g.rw, g.rh); return 1; }
            walks++;
        }
        for (int dtype = RGB_U8; dtype <= RGB_BF16; dtype++)
            for (int planar = 0; planar < 2; planar++)
                for (int mis = 0; mis < 2; mis++) {                                  // mis: the frame starts one sample behind the allocation's start
                    const int sz = dtype == RGB_U8 ? 1 : (dtype == RGB_F32 ? 4 : 2);
                    const size_t n = (size_t)3 * g.tw * g.th * sz;
                    std::unique_ptr<uint8_t[]> dst(new uint8_t[n + (mis ? sz : 0)]);
                    RgbJob rj = {};
                    rj.s = sj; rj.s.dst = dst.get() + (mis ? sz : 0); rj.s.out_fmt = 0;
                    rj.identity = g.rw == g.cw && g.rh == g.ch;
                    if (rj.identity) for (ScaleAxis &a : rj.s.ax) a = ScaleAxis{};        // (an identity job must not read tables: null ones)
                    rj.cy = 19077; rj.crv = 29372; rj.cgu = 3494; rj.cgv = 8731; rj.cbu = 34610; rj.yo = 16;      // BT.709, limited range
                    rj.dtype = dtype; rj.planar = planar; rj.bgr = mis; rj.fill = 0x123456;
                    for (int k = 0; k < 3; k++) { rj.k[k] = (1.0f / 255.0f) * (1.0f / 16384.0f); rj.b[k] = -0.5f; }
                    if (!walk::placed_rgb_frame(rj)) { fprintf(stderr, "%dx%d -> %dx%d: row guard (rgb)\n", g.cw, g.ch, g.rw, g.rh); return 1; }
                    walks++;
                }
    }
    printf("ok: %d walks over %d placements\n", walks, (int)(sizeof kGeos / sizeof kGeos[0]));
    return 0;
}
