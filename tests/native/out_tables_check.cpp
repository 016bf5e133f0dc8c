// tests/native/out_tables_check.cpp -- jmcodec_amd/csrc/out_tables.h behind a C ABI for tests/test_out_tables.py.  Test infrastructure only.
#include "../../jmcodec_amd/csrc/out_tables.h"
#include <string.h>

// the grid functions live beside the kernels in the product; here: any three functions the test can restate (only the maxima over them are checked)
namespace jmamd {
int scale_tiles(int tw, int th) { return 3 * tw + th; }
int rgb_tiles(int tw, int th) { return tw + 5 * th; }
int deint_items(int w, int h) { return w * h / 8; }
}
using namespace jmamd;

static uint8_t *ptr(int64_t v) { return (uint8_t *)(uintptr_t)v; }
static int64_t num(const uint8_t *p) { return (int64_t)(uintptr_t)p; }

extern "C" {
int ot_max_batch() { return kMaxBatch; }
// pics: n_pics x {disp_w, disp_h, pack_bytes, deint_bytes}.  rows, in the order the decoder queued them: n_rows x {pic, side, kind (0 plain, 1 scale, 2 rgb,
// 3 deint), dst, src, a, b, c, feeds, index} with a / b = width / height (plain, deint) or target width / height (scale, rgb), c = identity (rgb) or
// dst_pitch (deint).  scratch: base address, 0 = none.
// out: the four tables as they stand afterwards, 4 x (4 * kMaxBatch) x {dst, src, a, b} (all ones: never written).
// info: counts[kind * 2 + side] (8), max_w, max_h, s_tiles, r_tiles[0], r_tiles[1], d_items, alg_pack, alg_rgb, alg_deint, n_frames, n_rgb, n_deint,
// scratch_used, sum of bytes_needed, sum of frames().  ok: add()'s result per picture and side.
void ot_run(const int64_t *pics, int n_pics, const int64_t *rows, int n_rows, int64_t scratch, int64_t *out, int64_t *info, int64_t *ok) {
    const int cap = 4 * kMaxBatch;
    std::vector<PackJob> hp(cap); std::vector<ScaleJob> hs(cap); std::vector<RgbJob> hr(cap); std::vector<DeintJob> hd(cap);
    memset(hp.data(), 0xFF, sizeof(PackJob) * cap); memset(hs.data(), 0xFF, sizeof(ScaleJob) * cap);
    memset(hr.data(), 0xFF, sizeof(RgbJob) * cap); memset(hd.data(), 0xFF, sizeof(DeintJob) * cap);
    OutTables t;
    t.plain.host = hp.data(); t.scale.host = hs.data(); t.rgb.host = hr.data(); t.deint.host = hd.data();
    std::vector<OutSide> sides((size_t)n_pics * 2);
    for (int k = 0; k < n_rows; k++) {
        const int64_t *r = rows + 10 * k;
        OutSide &o = sides[(size_t)r[0] * 2 + r[1]];
        if (r[2] == 0) { PackJob j = {}; j.dst = ptr(r[3]); j.src = ptr(r[4]); j.width = (int)r[5]; j.height = (int)r[6]; o.plain.push_back(j); }
        if (r[2] == 1) { ScaleJob j = {}; j.dst = ptr(r[3]); j.src = ptr(r[4]); j.tw = (int)r[5]; j.th = (int)r[6]; o.scale.push_back(j); }
        if (r[2] == 2) { RgbJob j = {}; j.s.dst = ptr(r[3]); j.s.src = ptr(r[4]); j.s.tw = (int)r[5]; j.s.th = (int)r[6]; j.identity = (int)r[7]; o.rgb.push_back(j); }
        if (r[2] == 3) { DeintReq q = {}; q.job.dst = ptr(r[3]); q.job.src = ptr(r[4]); q.job.width = (int)r[5]; q.job.height = (int)r[6];
            q.job.dst_pitch = (int)r[7]; q.feeds = (int)r[8]; q.index = (int)r[9]; o.deint.push_back(q); }
    }
    int64_t need = 0, frames = 0;
    for (auto &o : sides) { need += (int64_t)OutTables::bytes_needed(o); frames += (int64_t)o.frames(); }
    t.reset(ptr(scratch));
    for (int i = 0; i < n_pics; i++) for (int side = 0; side < 2; side++)
        ok[2 * i + side] = t.add(sides[(size_t)i * 2 + side], side, (int)pics[4 * i], (int)pics[4 * i + 1], pics[4 * i + 2], pics[4 * i + 3]);
    for (int e = 0; e < cap; e++) {
        int64_t *p = out + 4 * e, *s = out + 4 * (cap + e), *r = out + 4 * (2 * cap + e), *d = out + 4 * (3 * cap + e);
        p[0] = num(hp[e].dst); p[1] = num(hp[e].src); p[2] = hp[e].width; p[3] = hp[e].height;
        s[0] = num(hs[e].dst); s[1] = num(hs[e].src); s[2] = hs[e].tw; s[3] = hs[e].th;
        r[0] = num(hr[e].s.dst); r[1] = num(hr[e].s.src); r[2] = hr[e].s.tw; r[3] = hr[e].s.th;
        d[0] = num(hd[e].dst); d[1] = num(hd[e].src); d[2] = hd[e].width; d[3] = hd[e].height;
    }
    for (int side = 0; side < 2; side++) { info[0 + side] = t.plain.n[side]; info[2 + side] = t.scale.n[side]; info[4 + side] = t.rgb.n[side];
        info[6 + side] = t.deint.n[side]; }
    const int64_t rest[] = {t.max_w, t.max_h, t.s_tiles, t.r_tiles[0], t.r_tiles[1], t.d_items, t.alg_pack, t.alg_rgb, t.alg_deint, t.n_frames, t.n_rgb,
        t.n_deint, (int64_t)t.scratch_used, need, frames};
    memcpy(info + 8, rest, sizeof rest);
}
}
