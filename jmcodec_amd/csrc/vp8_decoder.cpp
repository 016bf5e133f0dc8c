// jmcodec_amd/csrc/vp8_decoder.cpp -- the VP8 half of jmamd::Decoder (codec_type 5 = NV_CODEC_VP8, nv_dec/nv_dec.h:37-46 of the reference): key frames,
// and with option vp8_inter inter frames.
//
// The input is an IVF byte stream in any chunking, or one whole frame per call (Vp8Splitter, vp8_syntax.h).  The caller thread reads a frame's first
// ten bytes -- refusals and size changes are decided there (INTEGRATION.md "VP8") -- and picks a surface; a parse worker runs the bool decoder over
// the first partition and the token partitions into the job list (vp8_jobs.h); the engine runs k_vp8_recon and k_vp8_filter on the lane MJPEG and
// MPEG-2 ride and packs the picture out behind them.  A key frame references nothing: surfaces are dealt round robin as for MJPEG, frames leave in
// decode order, a frame with show_frame 0 is decoded and not handed out.  Job slots, output slots and the hand-over to the engine are shared with the
// other codecs (decoder.cpp).
//
// Option vp8_inter.  Last, golden and altref are three slots of the surface pool, held by index and never copied: a frame's header says which of them
// the frame becomes and which take over another's picture (vp8_update_refs, RFC 6386 9.7).  The round robin deals over kMaxSurfaces = 20 slots and
// skips the up to three that are references.  A slot it deals was dealt last at least 20 - 3 = 17 frames ago (every other slot that is no reference
// comes first) and stopped being a reference before this frame; pictures of a handle complete in order on one lane and hold one of at most
// kJpegJobSlots = 16 job slots from dispatch until their pack-out is done -- so the frame that was decoded into the slot, every frame that read it as
// a reference, and the display or pack-out it was owed have all completed, or run ahead of this frame on the same in-order stream (the readers).
// A golden frame therefore survives any number of frames, and nothing is copied.  The frame's references go to the engine as ref_mask: a further
// picture of the stream joins a batch only when it references nothing the batch writes (Engine::form), so a frame's references are complete when its
// launch starts.  The stream's frames are parsed in order on the caller thread (decoder.cpp push_task): the parse of frame n + 1 starts from the
// probabilities, the segment map and the deltas frame n left (Vp8State), and the reference flags sit in the bool-coded header.
#include "decoder.h"
#include "engine.h"
#include "vp8_jobs.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstring>

namespace jmamd {

void Decoder::vp8_feed(const uint8_t *buf, size_t len) {
    v8split_.feed(buf, len, [&](const uint8_t *p, size_t n, bool truncated) { if (!failed_) vp8_handle_frame(p, n, truncated); });
}

// end of stream: an IVF frame the stream ends inside is decoded as far as it goes (errors counts it)
void Decoder::vp8_flush() {
    const bool dropped = v8split_.flush([&](const uint8_t *p, size_t n, bool truncated) { if (!failed_) vp8_handle_frame(p, n, truncated); });
    if (dropped) { stat_errors_++; note_error("VP8: the stream ends inside an IVF header"); }
}

bool Decoder::vp8_activate(const Vp8FrameTag &tag) {
    bool changed = !seq_active_ || tag.width != v8_w_ || tag.height != v8_h_;
    const int dw = (tag.width + 1) & ~1, dh = (tag.height + 1) & ~1;      // an odd size: the even size just above is handed out, as for MJPEG
    // RFC 6386 9.2: color_space 0 is ITU-R BT.601 YUV -- the 601 coefficients, limited range (color_space 1 is recorded and changes nothing)
    { const int vui[4] = {0, -1, -1, 6}; resolve_color(vui, dh); }
    sar_[0] = sar_[1] = 0;
    // chroma centred both ways (location 1): the RFC is silent; libwebp derives a chroma sample as the mean of its 2x2 luma positions and upsamples accordingly
    if (resolve_chroma_loc(-1, -1, 1)) changed = true;
    if (!changed) return true;
    if (seq_active_) {
        // a new size starts a new sequence, like an SPS change: drain everything that still refers to the old surfaces
        auto t = std::make_unique<PicTask>();
        t->out_before = std::move(carry_out_); carry_out_.clear();
        push_task(std::move(t));
        { std::unique_lock<std::mutex> lk(mtx_); cv_.wait(lk, [&] { return outstanding_ == 0 && parse_pending_ == 0; }); }
        if (gpu_open_) { hipSetDevice(device_); free_surfaces(); free_job_buffers(); free_out_slots(false); }
        else free_job_buffers();
    }
    v8_w_ = tag.width; v8_h_ = tag.height;
    disp_w_ = dw; disp_h_ = dh;
    mb_w_ = (tag.width + 15) / 16; mb_h_ = (tag.height + 15) / 16;
    n_surf_ = vp8_inter_ ? kMaxSurfaces : kJpegSurfaces; extra_surf_ = 0; j_surf_rr_ = 0;      // (the round-robin rule and its argument: jpeg_decoder.cpp, and above)
    v8_ref_[0] = v8_ref_[1] = v8_ref_[2] = -1;
    for (auto &d : dpb_) d = DpbPic();
    if (n_jobs_set_) n_jobs_ = std::min(n_jobs_, kJpegJobSlots);
    if (!gpu_alloc_sequence()) return false;
    display_delay_ = std::min(display_delay_, n_jobs_ - 4);
    seq_active_ = true;
    if (!timer_started_) { t0_ = std::chrono::steady_clock::now(); timer_started_ = true; }
    return true;
}

void Decoder::vp8_handle_frame(const uint8_t *p, size_t n, bool truncated) {
    if (n == 0) { stat_v8_empty_++; return; }                  // (an IVF frame of size 0: a dropped frame; skipped and counted)
    auto vt = std::make_unique<Vp8Task>();
    const std::string e = vp8_read_tag(p, n, v8_key_seen_ == 0, vt->tag, vp8_inter_ != 0);
    if (!e.empty()) { stat_errors_++; fail(e); return; }
    if (truncated) { stat_errors_++; note_error("VP8: the stream ends inside a frame"); }
    const bool key = vt->tag.key;
    if (!key) { vt->tag.width = v8_w_; vt->tag.height = v8_h_; }       // (an inter frame has the size of the key frame before it)
    if (!vp8_activate(vt->tag)) return;
    if (key) v8_key_seen_++;
    vt->data.assign(p, p + n); vt->truncated = truncated;
    const bool show = vt->tag.show != 0;
    int slot = (int)(j_surf_rr_++ % (unsigned)n_surf_);
    while (slot == v8_ref_[0] || slot == v8_ref_[1] || slot == v8_ref_[2]) slot = (int)(j_surf_rr_++ % (unsigned)n_surf_);      // (option vp8_inter: above)
    vt->inter = !key;
    if (!key) for (int k = 0; k < 3; k++) vt->ref_slot[k] = v8_ref_[k];
    DpbPic &c = dpb_[slot];
    c = DpbPic(); c.decode_idx = decode_count_; c.poc = decode_count_;
    c.color = color_matrix_ | color_range_ << 4;
    c.deint = deint_when_ == 1;                          // (a VP8 frame is progressive: deinterlaced only on request, auto never fires)
    auto t = std::make_unique<PicTask>();
    t->has_picture = true; t->cur_slot = slot;
    t->out_before = std::move(carry_out_); carry_out_.clear();
    if (show) { t->out_after.push_back(display_entry(slot)); display_pocs_.push_back(decode_count_); c.out_at = decode_count_; }
    decode_count_++;
    if (key) { stat_i_++; stat_v8_key_++; } else { stat_p_++; stat_v8_inter_++; }
    if (!show) stat_v8_hidden_++;
    t->vp8 = std::move(vt);
    first_sh_ = SliceHeader(); first_sh_.type = key ? SL_I : SL_P;
    t->job_slot = acquire_job_slot();
    push_task(std::move(t));
}

// RFC 6386 9.7, in this order: the buffer copies (to altref, then to golden, both from the references
// as they were before this frame), then refresh_golden / refresh_alternate, then refresh_last.  A key frame becomes all three.
void Decoder::vp8_update_refs(const Vp8Pic &pic, int cur) {
    if (pic.tag.key) { v8_ref_[0] = v8_ref_[1] = v8_ref_[2] = cur; return; }
    const int last = v8_ref_[0], golden = v8_ref_[1], alt = v8_ref_[2];
    if (pic.copy_to_alt == 1) v8_ref_[2] = last; else if (pic.copy_to_alt == 2) v8_ref_[2] = golden;
    if (pic.copy_to_golden == 1) v8_ref_[1] = last; else if (pic.copy_to_golden == 2) v8_ref_[1] = alt;
    if (pic.refresh_golden) v8_ref_[1] = cur;
    if (pic.refresh_alt) v8_ref_[2] = cur;
    if (pic.refresh_last) v8_ref_[0] = cur;
}

// worker (option vp8_inter: the caller thread, frame after frame): bool-decode one frame and pack its job list
void Decoder::vp8_parse_task(PicTask *t) {
    auto pt0 = std::chrono::steady_clock::now();
    Vp8Task &vt = *t->vp8;
    JobSlot &js = jobs_[t->job_slot];
    static thread_local Vp8Pic pic;
    pic.tag = vt.tag;
    vp8_decode_frame(vt.data.data(), vt.data.size(), pic, vp8_inter_ ? &v8_state_ : nullptr);
    if (vp8_inter_) vp8_update_refs(pic, t->cur_slot);
    std::vector<uint8_t>().swap(vt.data);
    if (pic.damaged && !vt.truncated) { stat_errors_++; note_error("VP8: a partition runs past the end of the frame (damaged or truncated frame)"); }
    // the host validates every field the device indexes with; a list that fails is a bug of the parser, and the handle fails rather than launch it
    const std::string bad = vp8_validate_jobs(pic);
    if (!bad.empty()) { t->error = bad; fail(bad); pic.mbs.assign(pic.mbs.size(), Vp8Mb()); pic.entries.clear(); pic.split.clear(); pic.intra_mbs = (int)pic.mbs.size(); }
    vt.interp = pic.tag.version == 0 ? 0 : 1; vt.n_intra = pic.intra_mbs; vt.n_split = (int)pic.split.size(); vt.n_inter = (int)pic.mbs.size() - pic.intra_mbs;
    if (vt.inter) { stat_v8_golden_ += pic.golden_mbs; stat_v8_altref_ += pic.alt_mbs; stat_v8_split_ += pic.split_mbs; stat_v8_intra_in_inter_ += pic.intra_mbs; }
    vt.filter_type = pic.filter_type; vt.sharpness = pic.sharpness; vt.filtered = pic.filtered; memcpy(vt.dq, pic.dq, sizeof vt.dq);
    stat_v8_parts_ = pic.n_parts; stat_v8_filter_ = pic.filter_type; stat_v8_color_ = pic.color_space | pic.clamping << 1;
    if (pic.tag.key) stat_v8_scale_ = pic.tag.hscale | pic.tag.vscale << 2;
    { int s = 0; for (int k = 0; k < 4; k++) s += pic.segments_used >> k & 1; stat_v8_segments_ = s; }
    stat_v8_bpred_ += pic.bpred_mbs; stat_v8_skipped_ += pic.skipped_mbs;
    size_t off = 0;
    auto place = [&](size_t bytes) { size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; };
    vt.off_mbs = place(pic.mbs.size() * sizeof(Vp8Mb)); vt.off_entries = place(pic.entries.size() * 4);
    if (!pic.split.empty()) vt.off_split = place(pic.split.size() * sizeof(Vp8SplitMv));      // (a multiple of 16 bytes: nothing to pad)
    vt.n_entries = (int)pic.entries.size();
    t->n_slices = 1;
    if (!ensure_job_cap(js, off + 64)) fail("job buffer allocation failed");
    else {
        memcpy(js.host + vt.off_mbs, pic.mbs.data(), pic.mbs.size() * sizeof(Vp8Mb));
        if (!pic.entries.empty()) memcpy(js.host + vt.off_entries, pic.entries.data(), pic.entries.size() * 4);
        // the bytes that round each array up to 16 are uploaded and enter the job digest: zero, not what the allocation held
        memset(js.host + vt.off_mbs + pic.mbs.size() * sizeof(Vp8Mb), 0, vt.off_entries - vt.off_mbs - pic.mbs.size() * sizeof(Vp8Mb));
        memset(js.host + vt.off_entries + pic.entries.size() * 4, 0, (pic.split.empty() ? off : vt.off_split) - vt.off_entries - pic.entries.size() * 4);
        if (!pic.split.empty()) memcpy(js.host + vt.off_split, pic.split.data(), pic.split.size() * sizeof(Vp8SplitMv));
        t->upload_bytes = off;
        if (want_job_digest_) { uint64_t h = job_digest_; for (size_t i = 0; i < off; i++) { h ^= js.host[i]; h *= 1099511628211ull; } job_digest_ = h; }
        stat_pictures_++; stat_job_bytes_ += (long long)off; stat_coef_ += (long long)pic.entries.size(); stat_intra_mbs_ += (long long)pic.intra_mbs;
        if (!parse_only_ && !failed_) t->upload_seq = engine_->upload(js.dev, js.host, off, js.uploaded, false);
    }
    stat_parse_ns_i_ += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - pt0).count();
    t->state.store(1, std::memory_order_release);
    submit_ready();
    { std::lock_guard<std::mutex> lk(mtx_); parse_pending_--; cv_.notify_all(); }
}

// describe the picture to the device engine (called by submit_task)
void Decoder::vp8_fill_engine_pic(PicTask *t, EnginePic &ep) {
    const Vp8Task &vt = *t->vp8;
    JobSlot &js = jobs_[t->job_slot];
    ep.codec = 5; ep.uploaded = js.uploaded; ep.upload_seq = t->upload_seq;
    memset(&ep.hp, 0, sizeof ep.hp);
    ep.hp.cur = t->cur_slot;                             // (the engine's surface bookkeeping reads the slot here for every codec but H.264)
    Vp8PicParams &vp = ep.vp;
    memset(&vp, 0, sizeof vp);
    vp.surf = surf_[t->cur_slot]; vp.pitch = pitch_; vp.chroma_offset = chroma_off_;
    vp.mb_w = mb_w_; vp.mb_h = mb_h_;
    vp.n_entries = vt.n_entries; vp.filter_type = vt.filter_type; vp.sharpness = vt.sharpness; vp.filtered = vt.filtered ? 1 : 0;
    vp.mbs = (const Vp8Mb *)(js.dev + vt.off_mbs); vp.entries = (const uint32_t *)(js.dev + vt.off_entries);
    memcpy(vp.dq, vt.dq, sizeof vp.dq);
    if (vt.inter) {
        vp.inter = 1; vp.interp = vt.interp; vp.n_intra = vt.n_intra; vp.n_split = vt.n_split;
        vp.split = vt.n_split ? (const Vp8SplitMv *)(js.dev + vt.off_split) : nullptr;
        for (int k = 0; k < 3; k++) if (vt.ref_slot[k] >= 0 && vt.ref_slot[k] != t->cur_slot) { vp.ref[k] = surf_[vt.ref_slot[k]]; ep.ref_mask |= 1u << vt.ref_slot[k]; }
    }
    // algorithmic bytes: k_vp8_recon the job list in, 1.5 W H out; k_vp8_filter 1.5 W H in and out and the records
    const long long frame = (long long)mb_w_ * mb_h_ * 384;
    ep.vp8_recon_alg_bytes = (long long)t->upload_bytes + frame;
    ep.vp8_filter_alg_bytes = 2 * frame + (long long)mb_w_ * mb_h_ * (long long)sizeof(Vp8Mb);
    // k_vp8_inter: the job list and one reference sample per predicted sample in, the inter macroblocks out; k_vp8_recon then writes the intra ones only
    if (vt.inter) { ep.vp8_inter_alg_bytes = (long long)t->upload_bytes + 2LL * vt.n_inter * 384; ep.vp8_recon_alg_bytes = (long long)t->upload_bytes + (long long)vt.n_intra * 384; }
}

}  // namespace jmamd
