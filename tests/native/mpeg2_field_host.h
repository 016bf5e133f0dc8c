// tests/native/mpeg2_field_host.h -- the MPEG-2 host path with option mpeg2_field_pictures on, as one handle: mpeg2_decode_picture and
// mpeg2_reconstruct_host (the arithmetic k_mpeg2_recon runs) with the field pairing, reference field and lone-field rules of INTEGRATION.md "MPEG-2".
// Shared by tests/native/mpeg2_field_check.cpp (compared with the numpy restatement) and tools/mpeg2_field_asan.cpp (mutated streams under
// AddressSanitizer / UBSan: a surface is a heap block of exactly its size, so a read or a store outside it is caught).
#pragma once
#include "../../jmcodec_amd/csrc/mpeg2_syntax.h"
#include "../../jmcodec_amd/csrc/mpeg2_recon.h"
#include <cstring>
#include <memory>
#include <string>

using namespace jmamd;
static std::string g_err;

namespace {
struct Surface { std::vector<uint8_t> s; int w = 0, h = 0, W = 0, H = 0, have = 3; };      // NV12, pitch = W; have: bit 0 / 1 = top / bottom field decoded
struct Host {
    std::shared_ptr<Surface> anchor[2]; bool shown = true;
    std::shared_ptr<Surface> pend; int pend_par = 0, pend_type = 0;                       // the frame that waits for its second field
    Mpeg2Seq seq; bool have_seq = false;
    std::vector<std::shared_ptr<Surface>> out;
    int errors = 0, dropped = 0, clamped = 0, lone = 0, fields = 0, n_dual = 0, n_16x8 = 0, pictures = 0, max_mb = 0; bool refused = false;
    void show() { if (anchor[1] && !shown) { out.push_back(anchor[1]); shown = true; } }
    // the waiting first field stays alone: its lines are repeated into the missing field's, an error is counted, a B frame is displayed
    void close_pending() {
        if (!pend) return;
        Surface &f = *pend;
        const int e = pend_par;
        for (int y = 0; y < f.H / 2; y++) memcpy(&f.s[(size_t)(2 * y + 1 - e) * f.W], &f.s[(size_t)(2 * y + e) * f.W], (size_t)f.W);
        for (int y = 0; y < f.H / 4; y++) memcpy(&f.s[(size_t)f.W * f.H + (size_t)(2 * y + 1 - e) * f.W], &f.s[(size_t)f.W * f.H + (size_t)(2 * y + e) * f.W], (size_t)f.W);
        errors++; lone++;
        if (pend_type == 3) out.push_back(pend);
        pend.reset();
    }
    static const uint8_t *field_of(const std::shared_ptr<Surface> &f, int p) { return f ? f->s.data() + (size_t)p * f->W : nullptr; }
    void picture(Mpeg2Pic &pic) {
        if (refused) return;
        if (!pic.have_ext) { errors++; return; }
        const Mpeg2Seq &s = pic.seq;
        if (max_mb > 0 && (s.mb_w() > max_mb || s.mb_h() > max_mb)) return;               // (a mutated size field: keep the trial short)
        if (have_seq && (s.width != seq.width || s.height != seq.height || s.progressive_sequence != seq.progressive_sequence)) {
            close_pending(); show(); anchor[0].reset(); anchor[1].reset(); }
        seq = s; have_seq = true;
        if (pic.field() && s.progressive_sequence) { errors++; return; }                  // a damaged picture: skipped
        const int par = pic.picture_structure == 2 ? 1 : 0;
        const bool second = pend && pic.field() && par != pend_par &&
                            (pend_type == pic.type || (pend_type == 1 && pic.type == 2));
        if (pend && !second) close_pending();
        if (!second && ((pic.type == 2 && !anchor[1]) || (pic.type == 3 && (!anchor[0] || !anchor[1])))) { dropped++; return; }
        Mpeg2Jobs jobs; bool refuse = false;
        const std::string e = mpeg2_decode_picture(pic, jobs, &refuse);
        if (!e.empty()) { g_err = e; if (refuse) { refused = true; return; } errors++; }
        if (jobs.clamped) { clamped += jobs.clamped; errors++; }
        n_dual += jobs.n_dual; n_16x8 += jobs.n_16x8; fields += pic.field();
        std::shared_ptr<Surface> cur;
        if (second) { cur = pend; cur->have = 3; pend.reset(); }
        else {
            cur = std::make_shared<Surface>();
            cur->W = s.mb_w() * 16; cur->H = s.mb_h() * 16; cur->w = (s.width + 1) & ~1; cur->h = (s.height + 1) & ~1;
            cur->s.assign((size_t)cur->W * cur->H * 3 / 2, 0);
            if (pic.type != 3) { show(); anchor[0] = anchor[1]; anchor[1] = cur; shown = false; }       // (an anchor frame is the newer anchor from its first picture on)
            if (pic.field()) { cur->have = 1 << par; pend = cur; pend_par = par; pend_type = pic.type; }
        }
        Mpeg2PicParams pp = {};
        pp.surf = cur->s.data(); pp.pitch = cur->W; pp.chroma_offset = cur->W * cur->H; pp.mb_w = s.mb_w(); pp.mb_h = pic.mb_h();
        if (!pic.field()) {
            // (the anchors have moved already when this is an anchor: its reference is the anchor before it)
            pp.ref[0] = pic.type == 2 ? anchor[0]->s.data() : (pic.type == 3 ? anchor[0]->s.data() : nullptr);
            pp.ref[1] = pic.type == 3 ? anchor[1]->s.data() : nullptr;
        } else {
            pp.structure = pic.picture_structure;
            if (pic.type == 2) {          // 7.6.2.1: the two reference fields decoded last
                for (int p = 0; p < 2; p++) pp.fref[0][p] = field_of(anchor[0], p);
                if (second) pp.fref[0][1 - par] = field_of(cur, 1 - par);
            } else if (pic.type == 3) for (int p = 0; p < 2; p++) { pp.fref[0][p] = field_of(anchor[0], p); pp.fref[1][p] = field_of(anchor[1], p); }
        }
        pp.ext = pp.structure || jobs.n_dual || jobs.n_16x8;
        pp.n_entries = (int)jobs.entries.size(); pp.dc_mult = 8 >> pic.intra_dc_precision;
        pp.mbs = jobs.mbs.data(); pp.entries = jobs.entries.data();
        memcpy(pp.w, s.w, sizeof pp.w);
        mpeg2_reconstruct_host(pp);
        pictures++;
        if (pic.type == 3 && !pend) out.push_back(cur);
    }
};
}  // namespace

