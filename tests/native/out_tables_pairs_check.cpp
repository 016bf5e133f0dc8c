// tests/native/out_tables_pairs_check.cpp -- jmcodec_amd/csrc/out_tables.h with field-rate pairs behind a C ABI for tests/test_out_tables_pairs.py.
// Test infrastructure only.
#include "../../jmcodec_amd/csrc/out_tables.h"
#include <string.h>

namespace jmamd {
int scale_tiles(int tw, int th) { return 3 * tw + th; }
int rgb_tiles(int tw, int th) { return tw + 5 * th; }
int deint_items(int w, int h) { return w * h / 8; }
}
using namespace jmamd;

extern "C" {
// One picture, one side: n deinterlaced frames of a handle of `feeds` (0 plain, 1 scaled, 2 RGB), frame k a pair when pair[k] != 0, queued the way
// Decoder::enqueue_output queues them.  scratch: base address (0 = none).  out per frame: dst, dst2 of the k_deint job and the src of the one or two
// ScaleJobs / RgbJobs behind it (4 values).  info: deint entries, scale entries, rgb entries, pairs, n_deint, alg_deint, scratch_used, bytes_needed,
// frames(), add()'s result.
void otp_run(int n, const int *pair, int feeds, int w, int h, int pitch, int64_t scratch, int64_t deint_bytes, int64_t *out, int64_t *info) {
    const int cap = 4 * kMaxBatch;
    std::vector<PackJob> hp(cap); std::vector<ScaleJob> hs(cap); std::vector<RgbJob> hr(cap); std::vector<DeintJob> hd(cap);
    OutTables t;
    t.plain.host = hp.data(); t.scale.host = hs.data(); t.rgb.host = hr.data(); t.deint.host = hd.data();
    OutSide o;
    std::vector<int> first_job(n);
    for (int k = 0; k < n; k++) {
        uint8_t *slot1 = (uint8_t *)(uintptr_t)(0x1000000 + 0x10000 * (2 * k)), *slot2 = (uint8_t *)(uintptr_t)(0x1000000 + 0x10000 * (2 * k + 1));
        DeintReq r = {};
        r.job.src = (const uint8_t *)(uintptr_t)0x500000; r.job.width = w; r.job.height = h; r.job.dst_pitch = feeds ? pitch : w;
        if (!feeds) { r.job.dst = slot1; r.job.dst2 = pair[k] ? slot2 : nullptr; }
        else {
            r.feeds = feeds; r.index = (int)(feeds == 1 ? o.scale.size() : o.rgb.size()); r.index2 = pair[k] ? r.index + 1 : 0;
            first_job[k] = r.index;
            for (int c = 0; c < (pair[k] ? 2 : 1); c++) {
                if (feeds == 1) { ScaleJob j = {}; j.dst = c ? slot2 : slot1; j.tw = w; j.th = h; o.scale.push_back(j); }
                else { RgbJob j = {}; j.s.dst = c ? slot2 : slot1; j.s.tw = w; j.s.th = h; j.identity = 1; o.rgb.push_back(j); }
            }
        }
        o.deint.push_back(r);
    }
    t.reset((uint8_t *)(uintptr_t)scratch);
    const bool ok = t.add(o, kAfter, w, h, 1000, deint_bytes);
    int e = 0;
    for (int k = 0; k < n; k++) {
        int64_t *q = out + 4 * k;
        q[0] = q[1] = q[2] = q[3] = -1;
        if (scratch || !feeds) { const DeintJob &j = t.deint.h(kAfter)[e++]; q[0] = (int64_t)(uintptr_t)j.dst; q[1] = (int64_t)(uintptr_t)j.dst2; }
        if (feeds) for (int c = 0; c < (pair[k] ? 2 : 1); c++)
            q[2 + c] = (int64_t)(uintptr_t)(feeds == 1 ? t.scale.h(kAfter)[first_job[k] + c].src : t.rgb.h(kAfter)[first_job[k] + c].s.src);
    }
    const int64_t v[] = {t.deint.n[kAfter], t.scale.n[kAfter], t.rgb.n[kAfter], t.pairs[kAfter], t.n_deint, t.alg_deint, (int64_t)t.scratch_used,
        (int64_t)OutTables::bytes_needed(o), (int64_t)o.frames(), ok};
    memcpy(info, v, sizeof v);
}
}
