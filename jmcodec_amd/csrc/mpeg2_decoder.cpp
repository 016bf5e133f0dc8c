// jmcodec_amd/csrc/mpeg2_decoder.cpp -- the MPEG-2 half of jmamd::Decoder (codec_type 4 = NV_CODEC_MPEG2, nv_dec/nv_dec.h:37-46 of the reference).
//
// The input is any chunking of an ISO/IEC 13818-2 video elementary stream.  The caller thread cuts it at start codes, reads the headers and
// reassembles pictures (Mpeg2Splitter; what is accepted, what fails the handle: INTEGRATION.md "MPEG-2"), keeps the two anchor pictures and the
// display order, and picks a surface; a parse worker runs the slice / macroblock VLC decode into the job list (mpeg2_jobs.h); the engine runs
// k_mpeg2_recon on the HEVC lane and packs the display frames out behind it.  Job slots, output slots and the hand-over to the engine are shared
// with the other codecs (decoder.cpp).
#include "decoder.h"
#include "engine.h"
#include "mpeg2_jobs.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstring>

namespace jmamd {

// Two anchors and the picture being decoded are held by the stream itself; the rest lets pictures stay in flight: a surface is free once it is
// neither an anchor nor waiting for its pack-out, and the cold ones (displayed two pictures ago or earlier) are taken first, as for HEVC.  The
// engine orders every writer of a surface behind the batches that read or display it.
constexpr int kMpeg2Surfaces = 8;

void Decoder::mpeg2_feed(const uint8_t *buf, size_t len) {
    m2split_.feed(buf, len, [&](Mpeg2Pic &p) { if (!failed_) mpeg2_handle_picture(p); });
    mpeg2_after_split();
}

// end of stream: the picture in progress is decoded as far as its slices go
void Decoder::mpeg2_flush() {
    m2split_.flush([&](Mpeg2Pic &p) { if (!failed_) mpeg2_handle_picture(p); });
    if (!failed_) mpeg2_close_pending();
    mpeg2_after_split();
}

void Decoder::mpeg2_after_split() {
    if (m2split_.damaged_headers > m2_damaged_seen_) {
        stat_errors_ += m2split_.damaged_headers - m2_damaged_seen_; m2_damaged_seen_ = m2split_.damaged_headers;
        note_error("MPEG-2: a damaged header was skipped");
    }
    if (m2split_.refused() && !failed_) { stat_errors_++; fail(m2split_.error()); }
}

// the newer anchor leaves for display: when the next anchor arrives, at a new sequence, at the flush.  at: the decode index it is displayed behind
void Decoder::mpeg2_show_anchor(std::vector<int> &out) {
    const int s = m2_anchor_[1];
    if (s < 0 || m2_anchor_shown_) return;
    out.push_back(display_entry(s)); display_pocs_.push_back(dpb_[s].poc);
    dpb_[s].out_at = decode_count_;
    m2_anchor_shown_ = true;
}

bool Decoder::mpeg2_activate(const Mpeg2Seq &s) {
    bool changed = !seq_active_ || s.width != m2seq_.width || s.height != m2seq_.height || s.progressive_sequence != m2seq_.progressive_sequence;
    // the colour description of a sequence_display_extension; without one the standard's default, matrix 1.  Limited range either way
    { const int vui[4] = {0, s.have_colour ? s.primaries : -1, s.have_colour ? s.transfer : -1, s.have_colour ? s.matrix : 1}; resolve_color(vui, (s.height + 1) & ~1); }
    s.sar(&sar_[0], &sar_[1]);
    // 4:2:0 of MPEG-2: chroma sited with the left luma column, between the lines (location 0)
    if (resolve_chroma_loc(-1, -1, 0)) changed = true;
    if (!changed) { m2seq_ = s; return true; }
    if (s.mb_w() > 1024 || s.mb_h() > 1056 || (long long)s.mb_w() * s.mb_h() > 139264) {
        stat_errors_++; fail("MPEG-2: a picture of " + std::to_string(s.width) + "x" + std::to_string(s.height) + " is larger than the handle's surfaces carry");
        return false;
    }
    if (seq_active_) {
        // a new size starts a new sequence, like an SPS change: the last anchor is displayed, then everything that refers to the old surfaces drains
        mpeg2_close_pending();
        mpeg2_show_anchor(carry_out_);
        auto t = std::make_unique<PicTask>();
        t->out_before = std::move(carry_out_); carry_out_.clear();
        push_task(std::move(t));
        { std::unique_lock<std::mutex> lk(mtx_); cv_.wait(lk, [&] { return outstanding_ == 0 && parse_pending_ == 0; }); }
        if (gpu_open_) { hipSetDevice(device_); free_surfaces(); free_job_buffers(); free_out_slots(false); }
        else free_job_buffers();
    }
    m2seq_ = s;
    disp_w_ = (s.width + 1) & ~1; disp_h_ = (s.height + 1) & ~1;
    mb_w_ = s.mb_w(); mb_h_ = s.mb_h();
    n_surf_ = kMpeg2Surfaces; extra_surf_ = 0;
    for (auto &d : dpb_) d = DpbPic();
    m2_anchor_[0] = m2_anchor_[1] = -1; m2_anchor_shown_ = true; m2_pend_slot_ = -1;
    if (n_jobs_set_) n_jobs_ = std::min(n_jobs_, kJpegJobSlots);
    if (!gpu_alloc_sequence()) return false;
    display_delay_ = std::min(display_delay_, n_jobs_ - 4);
    seq_active_ = true;
    if (!timer_started_) { t0_ = std::chrono::steady_clock::now(); timer_started_ = true; }
    return true;
}

// Option mpeg2_field_pictures: the first field picture of a frame waits for its second one.  Whatever comes instead -- a frame picture, a field of
// the same parity or of a type that does not pair, a new sequence, the flush -- leaves it a lone field: `errors` counts it, its frame is displayed
// through the lone-field entry (DpbPic::lone: its lines repeated, bob when deinterlacing), a B frame right away, an anchor in its turn.  A lone
// anchor's missing field is then WRITTEN -- a picture of its own without coded data (Mpeg2Task::fill: every macroblock a zero-vector copy of the
// field that exists) -- so that whatever references the frame later, frame pictures included, reads the existing field's lines in both parities.
void Decoder::mpeg2_close_pending() {
    const int slot = m2_pend_slot_;
    if (slot < 0) return;
    m2_pend_slot_ = -1;
    DpbPic &c = dpb_[slot];
    c.lone = m2_pend_par_ + 1;
    stat_errors_++; stat_m2_lone_++;
    note_error("MPEG-2: a first field picture without its second field");
    // (the frame leaves in front of the NEXT picture, whose decode index decode_count_ is: its surface cools from there, as a B frame's does from its own)
    if (m2_pend_type_ == 3) { carry_out_.push_back(display_entry(slot)); display_pocs_.push_back(c.poc); c.out_at = decode_count_; return; }
    auto mt = std::make_unique<Mpeg2Task>();
    mt->fill = true; mt->structure = 2 - m2_pend_par_;                        // the parity that is missing
    mt->pic.seq = m2seq_; mt->pic.type = 2; mt->pic.picture_structure = mt->structure;
    for (int p = 0; p < 2; p++) { mt->fref_slot[0][p] = slot; mt->fref_par[0][p] = m2_pend_par_; }
    auto t = std::make_unique<PicTask>();
    t->has_picture = true; t->cur_slot = slot;
    t->out_before = std::move(carry_out_); carry_out_.clear();
    t->mpeg2 = std::move(mt);
    t->job_slot = acquire_job_slot();
    push_task(std::move(t));
}

void Decoder::mpeg2_handle_picture(Mpeg2Pic &pic) {
    if (!pic.have_ext) { stat_errors_++; note_error("MPEG-2: a picture header without its picture coding extension was skipped"); return; }
    if (!mpeg2_activate(pic.seq)) return;
    const bool anchor = pic.type != 3, fieldpic = pic.field();
    if (fieldpic && pic.seq.progressive_sequence) { stat_errors_++; note_error("MPEG-2: a field picture in a progressive sequence was skipped"); return; }
    // a field picture is the second field of the waiting frame when it has the other parity and the types pair: I-I, I-P, P-P, B-B
    const int par = pic.picture_structure == 2 ? 1 : 0;
    const bool second = m2_pend_slot_ >= 0 && fieldpic && par != m2_pend_par_ && (m2_pend_type_ == pic.type || (m2_pend_type_ == 1 && pic.type == 2));
    if (m2_pend_slot_ >= 0 && !second) mpeg2_close_pending();
    // a P picture before the first I, a B picture without both of its anchors (the leading B pictures of an open group): dropped, not errors
    if (!second && ((pic.type == 2 && m2_anchor_[1] < 0) || (pic.type == 3 && (m2_anchor_[0] < 0 || m2_anchor_[1] < 0)))) { stat_dropped_++; return; }
    auto mt = std::make_unique<Mpeg2Task>();
    auto t = std::make_unique<PicTask>();
    int slot;
    if (second) {
        // the second field goes into the first one's surface.  Engine::form keeps a picture out of a batch that already writes its surface, so this
        // picture always runs in a later launch than the first field -- which a second P field reads (mpeg2_fill_engine_pic names the surface in ref_mask)
        slot = m2_pend_slot_; m2_pend_slot_ = -1;
    } else {
        // (a new anchor references the newer anchor at most: the older one, displayed when the newer one arrived, retires first)
        if (anchor && m2_anchor_[0] >= 0) dpb_[m2_anchor_[0]].in_use = false;
        int warm = -1; bool wait_pack = false;
        slot = -1;
        for (int i = 0; i < n_surf_; i++) if (slot_free(i)) { if (decode_count_ >= dpb_[i].out_at + 2) { slot = i; break; } if (warm < 0) warm = i; }
        if (slot < 0 && warm >= 0) { slot = warm; wait_pack = true; }
        if (slot < 0) { stat_errors_++; fail("MPEG-2: no free surface"); return; }
        DpbPic &c = dpb_[slot];
        c = DpbPic(); c.decode_idx = decode_count_; c.poc = decode_count_;
        c.color = color_matrix_ | color_range_ << 4;
        c.deint = deint_when_ == 1 || !pic.progressive_frame;        // auto: the pictures that say they are two fields
        // (the field first in time is the one the deinterlacer keeps: top_field_first of a frame picture, the field first in the stream of two field pictures)
        c.fpoc[0] = fieldpic ? par : (pic.top_field_first ? 0 : 1); c.fpoc[1] = 1 - c.fpoc[0];
        c.in_use = anchor;
        t->wait_prev_pack = wait_pack;
    }
    DpbPic &c = dpb_[slot];
    // references.  A frame picture: the anchor(s) before it.  A field picture (7.6.2.1): a P field the two reference fields decoded last -- both fields
    // of the newer anchor for the first field of a frame, the first field of its own frame and the same-parity field of the anchor before for the
    // second; a B field both fields of both anchors.  (An anchor frame becomes the newer anchor with its first picture: `older` is the anchor before it.)
    const int older = second && anchor ? m2_anchor_[0] : (anchor ? m2_anchor_[1] : m2_anchor_[0]);
    if (!fieldpic) {
        mt->ref_slot[0] = pic.type == 2 ? m2_anchor_[1] : (pic.type == 3 ? m2_anchor_[0] : -1);
        mt->ref_slot[1] = pic.type == 3 ? m2_anchor_[1] : -1;
    } else {
        mt->structure = pic.picture_structure;
        if (pic.type == 2) { for (int p = 0; p < 2; p++) mt->fref_slot[0][p] = older; if (second) mt->fref_slot[0][1 - par] = slot; }
        else if (pic.type == 3) for (int p = 0; p < 2; p++) { mt->fref_slot[0][p] = m2_anchor_[0]; mt->fref_slot[1][p] = m2_anchor_[1]; }
        stat_m2_fields_++;
    }
    t->has_picture = true; t->cur_slot = slot;
    t->out_before = std::move(carry_out_); carry_out_.clear();
    if (!second) {
        if (anchor) {                                            // the anchor before it is displayed now; this one when the next arrives, or at the flush
            mpeg2_show_anchor(t->out_after);
            m2_anchor_[0] = m2_anchor_[1]; m2_anchor_[1] = slot; m2_anchor_shown_ = false;
        }
        if (fieldpic) { m2_pend_slot_ = slot; m2_pend_par_ = par; m2_pend_type_ = pic.type; }
        decode_count_++;                                         // (display_poc and the decode index count frames)
    }
    if (!anchor && m2_pend_slot_ < 0) { t->out_after.push_back(display_entry(slot)); display_pocs_.push_back(c.poc); c.out_at = c.decode_idx; }
    (pic.type == 1 ? stat_i_ : (pic.type == 2 ? stat_p_ : stat_b_))++;
    if (pic.repeat_first_field) stat_m2_rff_++;                  // recorded; no frame is repeated
    first_sh_ = SliceHeader(); first_sh_.type = pic.type == 1 ? SL_I : (pic.type == 2 ? SL_P : SL_B);
    mt->pic = std::move(pic);
    t->mpeg2 = std::move(mt);
    t->job_slot = acquire_job_slot();
    push_task(std::move(t));
}

// worker: the slices of one picture into macroblock records and entries
void Decoder::mpeg2_parse_task(PicTask *t) {
    auto pt0 = std::chrono::steady_clock::now();
    Mpeg2Task &mt = *t->mpeg2;
    JobSlot &js = jobs_[t->job_slot];
    // option mpeg2_device_vlc: the device path, unless the handle wants the host-made lists (parse_only, the digests) or the prescan declines
    // With option mpeg2_field_pictures as well, decided from the picture header before the prescan: field pictures take the host path; frame pictures
    // stay on the device, where the lane decodes dual prime (Mpeg2VlcPic::dual_prime)
    if (mpeg2_dev_vlc_ && !mt.fill) {
        const bool host_only = mt.structure != 0;
        if (!host_only && !parse_only_ && !want_digest_ && !want_job_digest_ && mpeg2_parse_task_device(t)) return;
        stat_m2_host_pics_++;
    }
    static thread_local Mpeg2Jobs jobs;
    if (mt.fill) {
        // the missing field of a lone anchor field: zero-vector forward copies (both reference fields of the picture are the field that exists)
        Mpeg2Mb rec = {}; rec.flags = M2_FWD; rec.qscale = 2;
        jobs.mbs.assign((size_t)mt.pic.seq.mb_w() * (mt.pic.seq.mb_h() / 2), rec); jobs.entries.clear(); jobs.clamped = jobs.n_16x8 = jobs.n_dual = 0;
    } else {
        bool refuse = false;
        const std::string e = mpeg2_decode_picture(mt.pic, jobs, &refuse);
        if (!e.empty()) { t->error = e; stat_errors_++; if (refuse) fail(e); else note_error(e); }
        if (jobs.clamped) { stat_m2_clamped_ += jobs.clamped; stat_errors_++; note_error("MPEG-2: vectors that reach outside the reference picture were clamped"); }
        if (jobs.n_dual) stat_m2_dual_ += jobs.n_dual;           // (no locked add on the handle's shared line for a picture without any)
        if (jobs.n_16x8) stat_m2_16x8_ += jobs.n_16x8;
    }
    mt.ext = mt.structure != 0 || jobs.n_dual > 0 || jobs.n_16x8 > 0;
    std::vector<uint8_t>().swap(mt.pic.data);
    size_t off = 0;
    auto place = [&](size_t bytes) { size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; };
    mt.off_mbs = place(jobs.mbs.size() * sizeof(Mpeg2Mb)); mt.off_entries = place(jobs.entries.size() * 4);
    mt.n_entries = (int)jobs.entries.size();
    t->n_slices = 1;
    if (!ensure_job_cap(js, off + 64)) fail("job buffer allocation failed");
    else {
        memset(js.host, 0, off);
        memcpy(js.host + mt.off_mbs, jobs.mbs.data(), jobs.mbs.size() * sizeof(Mpeg2Mb));
        if (!jobs.entries.empty()) memcpy(js.host + mt.off_entries, jobs.entries.data(), jobs.entries.size() * 4);
        t->upload_bytes = off;
        if ((want_digest_ || want_job_digest_) && !mt.fill) {      // over the records and the entries (pictures are parsed in order: the digest option is synchronous)
            uint64_t h = m2_digest_; for (size_t i = 0; i < off; i++) { h ^= js.host[i]; h *= 1099511628211ull; }
            m2_digest_ = h; m2_digest_mbs_ += (long long)jobs.mbs.size();
            if (want_job_digest_) job_digest_ = h;
        }
        if (!mt.fill) stat_pictures_++;
        stat_job_bytes_ += (long long)off; stat_coef_ += (long long)jobs.entries.size();
        if (!parse_only_ && !failed_) t->upload_seq = engine_->upload(js.dev, js.host, off, js.uploaded, false);
    }
    (mt.pic.type == 1 ? stat_parse_ns_i_ : stat_parse_ns_p_) += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - pt0).count();
    t->state.store(1, std::memory_order_release);
    submit_ready();
    { std::lock_guard<std::mutex> lk(mtx_); parse_pending_--; cv_.notify_all(); }
}

// worker, option mpeg2_device_vlc: one pass over the picture's slices finds their first macroblock addresses; the VLC decode itself is k_mpeg2_vlc's
bool Decoder::mpeg2_parse_task_device(PicTask *t) {
    auto pt0 = std::chrono::steady_clock::now();
    Mpeg2Task &mt = *t->mpeg2;
    JobSlot &js = jobs_[t->job_slot];
    static thread_local Mpeg2SliceScan scan;
    if (!mpeg2_slice_scan(mt.pic, scan).empty()) return false;
    mt.on_device = true;
    // (the records are written on the device: a P frame picture that may hold dual prime asks for the kernel instantiation that knows it)
    mt.ext = mpeg2_field_pics_ && mt.pic.type == 2 && !mt.pic.frame_pred_frame_dct;
    std::vector<uint8_t>().swap(mt.pic.data);
    const size_t n_mbs = (size_t)mt.pic.seq.mb_w() * mt.pic.seq.mb_h();
    size_t off = 0;
    auto place = [&](size_t bytes) { size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; };
    // uploaded: the picture's parameters, the slice table, the slice bytes
    mt.off_par = place(sizeof(Mpeg2VlcPic)); mt.off_slices = place(scan.slices.size() * sizeof(Mpeg2Slice)); mt.off_bytes = place(scan.bytes.size());
    const size_t up = off;
    // device only: the records and the entries k_mpeg2_vlc writes and k_mpeg2_recon reads
    off = 0;
    mt.off_mbs = place(n_mbs * sizeof(Mpeg2Mb)); mt.off_entries = place((size_t)scan.n_entries * 4);
    const size_t dev_only = off;
    mt.n_entries = (int)scan.n_entries; mt.n_slices = (int)scan.slices.size();
    t->n_slices = 1;
    if (!ensure_job_cap(js, up + 64) || !ensure_dev_only(js, dev_only + 64)) fail("job buffer allocation failed");
    else {
        memset(js.host, 0, up);
        const Mpeg2VlcPic vp = mpeg2_vlc_pic(mt.pic);
        memcpy(js.host + mt.off_par, &vp, sizeof vp);
        memcpy(js.host + mt.off_slices, scan.slices.data(), scan.slices.size() * sizeof(Mpeg2Slice));
        memcpy(js.host + mt.off_bytes, scan.bytes.data(), scan.bytes.size());
        t->upload_bytes = up;
        stat_pictures_++; stat_job_bytes_ += (long long)up;
        stat_m2_dev_pics_++; stat_m2_dev_slices_ += (long long)scan.slices.size();
        if (!failed_) t->upload_seq = engine_->upload(js.dev, js.host, up, js.uploaded, false);
    }
    (mt.pic.type == 1 ? stat_parse_ns_i_ : stat_parse_ns_p_) += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - pt0).count();
    t->state.store(1, std::memory_order_release);
    submit_ready();
    { std::lock_guard<std::mutex> lk(mtx_); parse_pending_--; cv_.notify_all(); }
    return true;
}

// engine thread: what k_mpeg2_vlc reported for a device-path picture.  `errors` counts as mpeg2_parse_task counts: once for a picture with damage (or
// macroblocks no slice covers), once more for one with clamped vectors; the texts are the host path's.  Dual prime fails the handle, as on the host
// path -- but here the picture has been reconstructed (concealed from the dual-prime macroblock on) and frames of earlier pictures may be out already
void Decoder::mpeg2_device_status(const EnginePic &, const uint32_t *words) {
    const uint32_t damaged = words[0], kinds = words[1], clamped = words[2], flags = words[3];
    stat_m2_dev_damaged_ += damaged; if (flags >> 8) stat_m2_dual_ += flags >> 8;
    if (flags & 2) { stat_errors_++; fail(std::string("MPEG-2: ") + mpeg2_vlc_damage_text(kM2DmgDualPrime)); }
    else if (kinds) {
        int kind = 1; while (kind < kM2DmgKinds && !(kinds >> kind & 1)) kind++;
        stat_errors_++; note_error(std::string("MPEG-2: ") + mpeg2_vlc_damage_text(kind));
    } else if (flags & 1) { stat_errors_++; note_error("MPEG-2: macroblocks that no slice covers"); }
    if (clamped) { stat_m2_clamped_ += clamped; stat_errors_++; note_error("MPEG-2: vectors that reach outside the reference picture were clamped"); }
}

// describe the picture to the device engine (called by submit_task)
void Decoder::mpeg2_fill_engine_pic(PicTask *t, EnginePic &ep) {
    const Mpeg2Task &mt = *t->mpeg2;
    JobSlot &js = jobs_[t->job_slot];
    ep.codec = 4; ep.uploaded = js.uploaded; ep.upload_seq = t->upload_seq;
    memset(&ep.hp, 0, sizeof ep.hp);
    ep.hp.cur = t->cur_slot;                             // (the engine's surface bookkeeping reads the slot here for every codec but H.264)
    Mpeg2PicParams &mp = ep.mp;
    memset(&mp, 0, sizeof mp);
    mp.surf = surf_[t->cur_slot]; mp.pitch = pitch_; mp.chroma_offset = chroma_off_;
    int n_refs = 0;
    // (the independence rule of Engine::form: a picture stays out of a batch that writes one of the surfaces named here)
    for (int d = 0; d < 2; d++) if (mt.ref_slot[d] >= 0) { mp.ref[d] = surf_[mt.ref_slot[d]]; ep.ref_mask |= 1u << mt.ref_slot[d]; n_refs++; }
    // a field picture: the reference fields, per direction and parity.  A second P field names its own surface here, so it never shares a launch with
    // the first field of its frame (and Engine::form keeps it out of a batch that writes that surface in any case)
    mp.structure = mt.structure; mp.ext = mt.ext ? 1 : 0;
    if (mt.structure) for (int d = 0; d < 2; d++) {
        for (int p = 0; p < 2; p++) if (mt.fref_slot[d][p] >= 0) {
            mp.fref[d][p] = surf_[mt.fref_slot[d][p]] + (size_t)mt.fref_par[d][p] * pitch_; ep.ref_mask |= 1u << mt.fref_slot[d][p]; }
        if (mt.fref_slot[d][0] >= 0 || mt.fref_slot[d][1] >= 0) n_refs++;
    }
    const int rows = mt.structure ? mb_h_ / 2 : mb_h_;           // a field has half the frame's macroblock rows
    mp.mb_w = mb_w_; mp.mb_h = rows;
    mp.n_items = rows * ((mb_w_ + 3) / 4);
    mp.n_entries = mt.n_entries; mp.dc_mult = 8 >> mt.pic.intra_dc_precision;
    uint8_t *lists = mt.on_device ? js.dev_only : js.dev;        // (device path: written by k_mpeg2_vlc in front of k_mpeg2_recon; n_entries is the capacity)
    mp.mbs = (const Mpeg2Mb *)(lists + mt.off_mbs); mp.entries = (const uint32_t *)(lists + mt.off_entries);
    ep.mpeg2_on_device = mt.on_device;
    if (mt.on_device) {
        Mpeg2VlcParams &mv = ep.mv;
        memset(&mv, 0, sizeof mv);
        mv.n_slices = mt.n_slices;
        mv.pic = (const Mpeg2VlcPic *)(js.dev + mt.off_par); mv.slices = (const Mpeg2Slice *)(js.dev + mt.off_slices); mv.bytes = (const uint32_t *)(js.dev + mt.off_bytes);
        mv.mbs = (Mpeg2Mb *)(lists + mt.off_mbs); mv.entries = (uint32_t *)(lists + mt.off_entries);
        // algorithmic bytes of k_mpeg2_vlc: what was uploaded in, a record per macroblock out (the entries it writes are not known here)
        ep.mpeg2_vlc_alg_bytes = (long long)t->upload_bytes + 32ll * mb_w_ * mb_h_;
    }
    memcpy(mp.w, mt.pic.seq.w, sizeof mp.w);
    // algorithmic bytes: the job list in, the reference rows of each direction in, 1.5 W H out
    ep.mpeg2_alg_bytes = (long long)t->upload_bytes + (long long)(n_refs + 1) * mb_w_ * rows * 384;
}

}  // namespace jmamd
