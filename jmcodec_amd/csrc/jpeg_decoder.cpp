// jmcodec_amd/csrc/jpeg_decoder.cpp -- the MJPEG half of jmamd::Decoder (codec_type 2 = NV_CODEC_MJPEG, nv_dec/nv_dec.h:37-46 of the reference).
//
// The input is any chunking of a byte stream of concatenated JPEG interchange pictures.  The caller thread reassembles pictures (JpegSplitter), reads
// their headers (what is accepted, what fails the handle: INTEGRATION.md "MJPEG") and picks a surface; a parse worker runs the Huffman decode into the
// sparse job list (jpeg_jobs.h); the engine runs k_jpeg_recon on the HEVC lane and packs the picture out behind it.  A picture has no references:
// frames leave in decode order.  Job slots, output slots and the hand-over to the engine are shared with the other codecs (decoder.cpp).
#include "decoder.h"
#include "engine.h"
#include "jpeg_jobs.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstring>

namespace jmamd {

// A surface is written by k_jpeg_recon and read by the pack-out behind it; the picture holds its job slot until both are done, pictures of a handle
// complete in order (one lane), and at most kJpegJobSlots are in flight -- so handing surfaces out round robin over more of them than that never
// meets one that is still in use.
// (kJpegJobSlots = 16, kJpegSurfaces = 18: decoder.h)

void Decoder::jpeg_feed(const uint8_t *buf, size_t len) {
    jsplit_.feed(buf, len, [&](const uint8_t *p, size_t n, bool truncated) { if (!failed_) jpeg_handle_picture(p, n, truncated); });
}

// end of stream: a picture whose scan had begun is decoded as far as it goes (errors counts it)
void Decoder::jpeg_flush() {
    const bool dropped = jsplit_.flush([&](const uint8_t *p, size_t n, bool truncated) { if (!failed_) jpeg_handle_picture(p, n, truncated); });
    if (dropped) { stat_errors_++; note_error("MJPEG: the stream ends inside a picture's headers"); }
}

bool Decoder::jpeg_activate(const JpegPic &pic) {
    bool changed = !seq_active_ || pic.width != j_w_ || pic.height != j_h_ || pic.sampling != j_sampling_;
    // JFIF: BT.601 coefficients, full range
    { const int vui[4] = {1, -1, -1, 6}; resolve_color(vui, pic.disp_h()); }
    sar_[0] = sar_[1] = 0;
    // JFIF: chroma centred both ways (location 1), which is also what k_jpeg_recon's 4:2:2 / 4:4:4 -> 4:2:0 averaging produces
    if (resolve_chroma_loc(-1, -1, 1)) changed = true;
    if (!changed) return true;
    if (seq_active_) {
        // a new size or sampling starts a new sequence, like an SPS change: drain everything that still refers to the old surfaces
        auto t = std::make_unique<PicTask>();
        t->out_before = std::move(carry_out_); carry_out_.clear();
        push_task(std::move(t));
        { std::unique_lock<std::mutex> lk(mtx_); cv_.wait(lk, [&] { return outstanding_ == 0 && parse_pending_ == 0; }); }
        if (gpu_open_) { hipSetDevice(device_); free_surfaces(); free_job_buffers(); free_out_slots(false); }
        else free_job_buffers();
    }
    j_w_ = pic.width; j_h_ = pic.height; j_sampling_ = pic.sampling;
    disp_w_ = pic.disp_w(); disp_h_ = pic.disp_h();
    mb_w_ = (disp_w_ + 15) / 16; mb_h_ = (disp_h_ + 15) / 16;
    n_surf_ = kJpegSurfaces; extra_surf_ = 0; j_surf_rr_ = 0;
    for (auto &d : dpb_) d = DpbPic();
    // job slots: the caller's choice up to kJpegJobSlots, else gpu_alloc_sequence's (kJpegJobSlots, fewer where RGB output slots would pass 1 GiB)
    if (n_jobs_set_) n_jobs_ = std::min(n_jobs_, kJpegJobSlots);
    // (the surfaces are filled with 128 when they are allocated: a grey sequence never writes its chroma)
    if (!gpu_alloc_sequence()) return false;
    display_delay_ = std::min(display_delay_, n_jobs_ - 4);
    seq_active_ = true;
    if (!timer_started_) { t0_ = std::chrono::steady_clock::now(); timer_started_ = true; }
    return true;
}

void Decoder::jpeg_handle_picture(const uint8_t *p, size_t n, bool truncated) {
    auto jt = std::make_unique<JpegTask>();
    bool refuse = false;
    const std::string e = jpeg_parse_picture(p, n, jtab_, jt->pic, &refuse);
    if (!e.empty()) { stat_errors_++; if (refuse) fail(e); else note_error(e); return; }
    if (truncated) { stat_errors_++; note_error("MJPEG: the stream ends inside a picture"); }
    if (!jpeg_activate(jt->pic)) return;
    jt->data.assign(p + jt->pic.scan_off, p + jt->pic.scan_end);
    jt->pic.scan_end -= jt->pic.scan_off; jt->pic.scan_off = 0;
    const int slot = (int)(j_surf_rr_++ % (unsigned)n_surf_);
    DpbPic &c = dpb_[slot];
    c = DpbPic(); c.decode_idx = decode_count_; c.poc = decode_count_;
    c.color = color_matrix_ | color_range_ << 4;
    c.deint = deint_when_ == 1;                          // (a JPEG picture says nothing about interlace: deinterlaced only on request)
    auto t = std::make_unique<PicTask>();
    t->has_picture = true; t->cur_slot = slot;
    t->out_before = std::move(carry_out_); carry_out_.clear();
    t->out_after.push_back(display_entry(slot)); display_pocs_.push_back(decode_count_);
    c.out_at = decode_count_;
    decode_count_++;
    stat_i_++; stat_jpeg_pics_++;
    if (jt->pic.restart_interval) stat_jpeg_ri_++;
    // option jpeg_device_entropy: 1 takes the pictures whose scan is at least two restart segments, 2 takes every picture (one without DRI is one segment)
    jt->on_device = jpeg_dev_entropy_ == 2 || (jpeg_dev_entropy_ == 1 && jt->pic.restart_interval > 0 && jpeg_expected_segments(jt->pic) >= 2);
    if (jt->on_device) { stat_jpeg_dev_pics_++; stat_jpeg_dev_segs_ += jpeg_expected_segments(jt->pic); } else if (jpeg_dev_entropy_) stat_jpeg_host_pics_++;
    t->jpeg = std::move(jt);
    first_sh_ = SliceHeader(); first_sh_.type = SL_I;
    t->job_slot = acquire_job_slot();
    push_task(std::move(t));
}

// worker: Huffman-decode one picture and pack its job list
void Decoder::jpeg_parse_task(PicTask *t) {
    auto pt0 = std::chrono::steady_clock::now();
    JpegTask &jt = *t->jpeg;
    JobSlot &js = jobs_[t->job_slot];
    if (jt.on_device) { jpeg_parse_task_device(t); return; }
    static thread_local JpegJobs jobs;
    const std::string e = jpeg_decode_scan(jt.pic, jt.data.data(), jt.data.size(), jobs);
    if (!e.empty()) { t->error = e; stat_errors_++; note_error(e); }
    std::vector<uint8_t>().swap(jt.data);
    size_t off = 0;
    auto place = [&](size_t bytes) { size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; };
    jt.off_first = place(jobs.first.size() * 4); jt.off_count = place(jobs.count.size()); jt.off_entries = place(jobs.entries.size() * 4);
    jt.n_entries = (int)jobs.entries.size();
    t->n_slices = 1;
    if (!ensure_job_cap(js, off + 64)) fail("job buffer allocation failed");
    else {
        if (!jobs.first.empty()) memcpy(js.host + jt.off_first, jobs.first.data(), jobs.first.size() * 4);
        if (!jobs.count.empty()) memcpy(js.host + jt.off_count, jobs.count.data(), jobs.count.size());
        if (!jobs.entries.empty()) memcpy(js.host + jt.off_entries, jobs.entries.data(), jobs.entries.size() * 4);
        // the bytes that round each array up to 16 are uploaded and enter the job digest: zero, as on the device path below, not what the allocation held
        memset(js.host + jt.off_first + jobs.first.size() * 4, 0, jt.off_count - jt.off_first - jobs.first.size() * 4);
        memset(js.host + jt.off_count + jobs.count.size(), 0, jt.off_entries - jt.off_count - jobs.count.size());
        memset(js.host + jt.off_entries + jobs.entries.size() * 4, 0, off - jt.off_entries - jobs.entries.size() * 4);
        t->upload_bytes = off;
        if (want_job_digest_) { uint64_t h = job_digest_; for (size_t i = 0; i < off; i++) { h ^= js.host[i]; h *= 1099511628211ull; } job_digest_ = h; }
        stat_pictures_++; stat_job_bytes_ += (long long)off; stat_coef_ += (long long)jobs.entries.size();
        if (!parse_only_ && !failed_) t->upload_seq = engine_->upload(js.dev, js.host, off, js.uploaded, false);
    }
    stat_parse_ns_i_ += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - pt0).count();
    t->state.store(1, std::memory_order_release);
    submit_ready();
    { std::lock_guard<std::mutex> lk(mtx_); parse_pending_--; cv_.notify_all(); }
}

// what only the device touches: no page-locked mirror (ensure_job_cap sizes both sides alike, which is right for what is uploaded)
bool Decoder::ensure_dev_only(JobSlot &js, size_t bytes) {
    if (bytes <= js.dev_only_cap) return true;
    const size_t cap = bytes + bytes / 2 + 4096;
    if (parse_only_ || !gpu_open_) { js.dev_only_cap = cap; return true; }           // (nothing reads it: only the size is kept)
    hipSetDevice(device_);
    uint8_t *d = nullptr;
    if (hipMalloc((void **)&d, cap) != hipSuccess) { (void)hipGetLastError(); return false; }
    // the slot belongs to the picture being parsed: nothing on the device refers to the old buffer any more (see acquire_job_slot)
    if (js.dev_only) hipFree(js.dev_only);
    js.dev_only = d; js.dev_only_cap = cap;
    return true;
}

// worker, option jpeg_device_entropy: one pass over the scan cuts it into clean segments; the Huffman decode itself is k_jpeg_entropy's
void Decoder::jpeg_parse_task_device(PicTask *t) {
    auto pt0 = std::chrono::steady_clock::now();
    JpegTask &jt = *t->jpeg;
    JobSlot &js = jobs_[t->job_slot];
    static thread_local JpegSegments segs;
    const std::string e = jpeg_segment_scan(jt.pic, jt.data.data(), jt.data.size(), segs);
    if (!e.empty()) { t->error = e; jt.host_error = true; stat_errors_++; note_error(e); }
    std::vector<uint8_t>().swap(jt.data);
    const size_t n_blocks = (size_t)jt.pic.n_blocks();
    size_t off = 0;
    auto place = [&](size_t bytes) { size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; };
    // uploaded: tables, segment table, clean bytes
    jt.off_tab = place(6 * sizeof(JpegDevHuff)); jt.off_segs = place(segs.segs.size() * sizeof(JpegSegment)); jt.off_bytes = place(segs.bytes.size());
    const size_t up = off;
    // device only: the three arrays k_jpeg_entropy writes and k_jpeg_recon reads
    off = 0;
    jt.off_first = place(n_blocks * 4); jt.off_count = place(n_blocks); jt.off_entries = place((size_t)segs.n_entries * 4);
    const size_t dev_only = off;
    jt.n_entries = (int)segs.n_entries; jt.n_segs = (int)segs.segs.size();
    t->n_slices = 1;
    if (!ensure_job_cap(js, up + 64) || !ensure_dev_only(js, dev_only + 64)) fail("job buffer allocation failed");
    else {
        jpeg_device_tables(jt.pic, (JpegDevHuff *)(js.host + jt.off_tab));
        memset(js.host + jt.off_tab + 6 * sizeof(JpegDevHuff), 0, jt.off_segs - jt.off_tab - 6 * sizeof(JpegDevHuff));
        if (!segs.segs.empty()) memcpy(js.host + jt.off_segs, segs.segs.data(), segs.segs.size() * sizeof(JpegSegment));
        memset(js.host + jt.off_segs + segs.segs.size() * sizeof(JpegSegment), 0, jt.off_bytes - jt.off_segs - segs.segs.size() * sizeof(JpegSegment));
        if (!segs.bytes.empty()) memcpy(js.host + jt.off_bytes, segs.bytes.data(), segs.bytes.size());
        memset(js.host + jt.off_bytes + segs.bytes.size(), 0, up - jt.off_bytes - segs.bytes.size());
        t->upload_bytes = up;
        if (want_job_digest_) { uint64_t h = job_digest_; for (size_t i = 0; i < up; i++) { h ^= js.host[i]; h *= 1099511628211ull; } job_digest_ = h; }
        stat_pictures_++; stat_job_bytes_ += (long long)up;
        if (!parse_only_ && !failed_) t->upload_seq = engine_->upload(js.dev, js.host, up, js.uploaded, false);
    }
    stat_parse_ns_i_ += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - pt0).count();
    t->state.store(1, std::memory_order_release);
    submit_ready();
    { std::lock_guard<std::mutex> lk(mtx_); parse_pending_--; cv_.notify_all(); }
}

// engine thread: what k_jpeg_entropy reported for a device-path picture.  Damage is contained per segment (INTEGRATION.md "MJPEG"); the picture is
// handed out, and counted in `errors` once -- not again when the segmenter had counted it already
void Decoder::on_jpeg_entropy_status(const EnginePic &p, uint32_t damaged, uint32_t kinds) {
    if (!damaged) return;
    stat_jpeg_dev_damaged_ += damaged;
    if (p.jpeg_host_error) return;
    stat_errors_++;
    note_error((kinds & (kJpegDamageCode | kJpegDamageCap)) ? "MJPEG: an invalid Huffman code (damaged picture)"
                                                           : "MJPEG: the entropy-coded data ends early (damaged or truncated picture)");
}

// describe the picture to the device engine (called by submit_task)
void Decoder::jpeg_fill_engine_pic(PicTask *t, EnginePic &ep) {
    const JpegTask &jt = *t->jpeg;
    JobSlot &js = jobs_[t->job_slot];
    ep.codec = 2; ep.uploaded = js.uploaded; ep.upload_seq = t->upload_seq;
    memset(&ep.hp, 0, sizeof ep.hp);
    ep.hp.cur = t->cur_slot;                             // (the engine's surface bookkeeping reads the slot here for every codec but H.264)
    JpegPicParams &jp = ep.jp;
    memset(&jp, 0, sizeof jp);
    jp.surf = surf_[t->cur_slot]; jp.pitch = pitch_; jp.chroma_offset = chroma_off_;
    jp.coded_w = mb_w_ * 16; jp.coded_h = mb_h_ * 16;
    jp.sampling = jt.pic.sampling;
    jp.y_bw = jt.pic.y_bw; jp.y_bh = jt.pic.y_bh; jp.c_bw = jt.pic.c_bw; jp.c_bh = jt.pic.c_bh;
    jp.n_items_y = ((jp.y_bw + 7) / 8) * jp.y_bh;
    jp.n_items = jp.n_items_y + ((jp.c_bw + 3) / 4) * jp.c_bh;
    jp.n_blocks = jt.pic.n_blocks(); jp.n_entries = jt.n_entries;
    uint8_t *lists = jt.on_device ? js.dev_only : js.dev;        // (device path: written by k_jpeg_entropy in front of k_jpeg_recon; n_entries is the capacity)
    jp.first = (const uint32_t *)(lists + jt.off_first); jp.count = lists + jt.off_count; jp.entries = (const uint32_t *)(lists + jt.off_entries);
    ep.jpeg_on_device = jt.on_device; ep.jpeg_host_error = jt.host_error;
    if (jt.on_device) {
        JpegEntropyParams &je = ep.je;
        memset(&je, 0, sizeof je);
        je.n_segs = jt.n_segs; je.geom = jpeg_scan_geom(jt.pic);
        je.tab = (const JpegDevHuff *)(js.dev + jt.off_tab); je.segs = (const JpegSegment *)(js.dev + jt.off_segs); je.bytes = (const uint32_t *)(js.dev + jt.off_bytes);
        je.first = (uint32_t *)(lists + jt.off_first); je.count = lists + jt.off_count; je.entries = (uint32_t *)(lists + jt.off_entries);
        // algorithmic bytes of k_jpeg_entropy: what was uploaded in, a record per block out (the entries it writes are not known here)
        ep.jpeg_entropy_alg_bytes = (long long)t->upload_bytes + 5ll * jt.pic.n_blocks();
    }
    memcpy(jp.q, jt.pic.q, sizeof jp.q);
    // algorithmic bytes: the job list in, 1.5 W H out
    ep.jpeg_alg_bytes = (long long)t->upload_bytes + (long long)disp_w_ * disp_h_ * 3 / 2;
}

}  // namespace jmamd
