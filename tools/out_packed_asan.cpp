// tools/out_packed_asan.cpp -- the lane routines of k_scale_pack and k_rgb_pack (jmcodec_amd/csrc/scale_packed.h, rgb_packed.h) walked on the CPU over
// a fixed handful of edge geometries, built with AddressSanitizer / UBSan (host sanitizers; `make -C tools out_packed_asan`).  Source and destination
// are heap buffers of exactly the surface's and the frame's size, so a read or write outside either aborts.  Nothing here touches a device.
#include "../tests/native/rgb_packed_walk.h"
#include <cstdio>
#include <memory>

using namespace jmamd;

struct Geo { int W, H, cx, cy, cw, ch, tw, th, lone; };
static const Geo kGeos[] = {
    {2, 2, 0, 0, 2, 2, 2, 2, 0},                 // the smallest frame, identity
    {2, 2, 0, 0, 2, 2, 8, 8, 0},                 // ... at 1:4
    {66, 18, 0, 0, 66, 18, 66, 18, 0},           // one tile plus one column pair / row pair, identity
    {132, 36, 0, 0, 132, 36, 66, 18, 1},         // ... as the target of a 2:1 downscale, top field alone
    {130, 34, 0, 0, 130, 34, 130, 34, 2},        // bottom field alone, H % 4 == 2: the last chroma row pair maps one row below the frame's chroma
    {130, 34, 0, 0, 130, 34, 96, 20, 2},
    {640, 272, 0, 0, 640, 272, 80, 34, 0},       // 8:1 in both directions
    {30, 14, 0, 0, 30, 14, 120, 56, 0},          // 1:4 in both directions
    {180, 100, 90, 50, 90, 50, 46, 74, 0},       // the crop ends at the right / bottom edge; down in x, up in y
    {180, 100, 90, 50, 90, 50, 90, 50, 1},       // ... identity
    {398, 298, 2, 4, 390, 290, 64, 48, 0},       // the target is exactly one luma tile wide
};

int main() {
    int walks = 0;
    for (const Geo &g : kGeos) {
        const int pitch = g.W;                                                      // tight rows: nothing behind a row's last sample but the next row
        const int hs = g.H + (g.lone && g.H % 4 ? 2 : 0);                            // surface rows: a lone field of H % 4 == 2 reads the next chroma row
        const size_t src_n = (size_t)pitch * hs * 3 / 2;
        std::unique_ptr<uint8_t[]> src(new uint8_t[src_n]);
        for (size_t i = 0; i < src_n; i++) src[i] = (uint8_t)(i * 131 + (i >> 8) * 17);
        walk::Tables tables;
        ScaleJob sj{src.get(), nullptr, pitch, pitch * hs, g.cx, g.cy, g.tw, g.th, 0, g.lone, {}};
        if (!tables.build(g.cw, g.ch, g.tw, g.th, sj.ax)) { fprintf(stderr, "%dx%d -> %dx%d: no tap tables\n", g.cw, g.ch, g.tw, g.th); return 1; }
        for (int fmt = 0; fmt < 2; fmt++) {
            std::unique_ptr<uint8_t[]> dst(new uint8_t[(size_t)g.tw * g.th * 3 / 2]);
            sj.dst = dst.get(); sj.out_fmt = fmt;
            if (!walk::scale_frame(sj)) { fprintf(stderr, "%dx%d -> %dx%d: row guard\n", g.cw, g.ch, g.tw, g.th); return 1; }
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
                    rj.identity = g.tw == g.cw && g.th == g.ch;
                    rj.cy = 19077; rj.crv = 29372; rj.cgu = 3494; rj.cgv = 8731; rj.cbu = 34610; rj.yo = 16;      // BT.709, limited range
                    rj.dtype = dtype; rj.planar = planar; rj.bgr = mis;
                    for (int k = 0; k < 3; k++) { rj.k[k] = (1.0f / 255.0f) * (1.0f / 16384.0f); rj.b[k] = -0.5f; }
                    if (!walk::rgb_frame(rj)) { fprintf(stderr, "%dx%d -> %dx%d: row guard (rgb)\n", g.cw, g.ch, g.tw, g.th); return 1; }
                    walks++;
                }
    }
    printf("ok: %d walks over %d geometries\n", walks, (int)(sizeof kGeos / sizeof kGeos[0]));
    return 0;
}
