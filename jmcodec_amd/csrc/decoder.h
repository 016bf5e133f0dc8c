// jmcodec_amd/csrc/decoder.h -- per-handle decode pipeline behind the jm_nvdec_* API.
//
// Re-implements nvdec_ctx and its call flow (/root/reference/nv_dec/nv_dec.h:69-126,
// nv_dec.cpp:62-80, :368-478, :496-540) without CUVID:
//   caller thread : Annex-B splitter -> SPS/PPS/slice headers -> POC, DPB, ref lists, display order
//   worker pool   : CAVLC slice_data() -> macroblock job list in a pinned buffer      (h264_cavlc.cpp)
//   HIP stream    : H2D job list -> k_recon_inter -> k_recon_intra -> k_deblock -> k_packout -> D2H
//   caller thread : jm_nvdec_output_frame = one memcpy out of the pinned output slot
#pragma once
#include "h264_cavlc.h"
#include "h264_syntax.h"
#include "hevc_slice.h"
#include "hevc_sei.h"
#include "jpeg_syntax.h"
#include "mpeg2_syntax.h"
#include "vp8_syntax.h"
#include "jobs.h"
#include "scale_packed.h"    // build_scale_taps
#include "chroma_packed.h"   // build_chroma_taps
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

struct ihipStream_t; struct ihipEvent_t;

namespace jmamd {

constexpr int kMaxJobSlots = 64;  // upper bound of the option "job_slots" / JM_AMD_DEC_JOB_SLOTS
constexpr int kJobSlots = 24;   // pictures in flight per handle (parse + device); deep enough to hide an I picture's entropy decode behind a GOP of device work
// H.264 streams up to 1080p: one stream alone is fed by what fits into its slots -- a chain launch holds n pictures while the next n are parsed, and a launch
// costs ~0.85 ms plus ~0.1 ms per picture, so n decides its rate: 24 slots -> 6.8 pictures per launch, 4.5 k frames/s; 40 slots (and chains of up to 16) ->
// 14.6 per launch, 6.6 k (profiles/r06_single_stream_slots.txt).  1.3 MB of page-locked memory per slot at 1080p Baseline
constexpr int kJobSlotsSmall = 40;
// MJPEG: pictures are independent and of one size, nothing like an I picture's parse has to hide behind a GOP; its surfaces are dealt round robin over
// kJpegSurfaces > kJpegJobSlots (jpeg_decoder.cpp), so a handle never runs more job slots than this, whatever "job_slots" asks for
constexpr int kJpegJobSlots = 16, kJpegSurfaces = 18;

struct DpbPic {                                // one frame store (C.4.5): a frame, or the one or two field pictures of a frame
    bool in_use = false;                       // NOT the test for a free surface: a surface may be free of a picture and still held for the next display
                                               // frame (Decoder::hold_) -- every place that hands out a surface asks Decoder::slot_free
    // marking.  fmark[]: each field (top, bottom): 0 not a reference, 1 short-term, 2 long-term.  ref is derived (sync_ref): 1 / 2 = BOTH fields so,
    // i.e. a reference FRAME in the sense of 8.2.4.2.1; 3 = some field is a reference (field pictures can use it, and the store stays occupied)
    int ref = 0; int fmark[2] = {0, 0};
    int fpoc[2] = {0, 0};                      // TopFieldOrderCnt, BottomFieldOrderCnt
    int have = 0;                              // bit 0 / 1: top / bottom field decoded (a frame picture: both)
    bool waiting_second = false, first_was_ref = false, coded_as_fields = false;
    bool non_existing = false;                 // a frame inferred from a gap in frame_num (8.2.5.2): a short-term reference without samples, never displayed
    int lone = 0;                              // set when the store is complete: 1 / 2 = only its top / bottom field was decoded
    int color = 0;                             // matrix | range << 4 of the sequence the picture was decoded in (RGB output)
    bool deint = false;                        // the picture's sequence is one whose frames are deinterlaced (option deinterlace_when)
    void set_ref(int v) { fmark[0] = fmark[1] = v; ref = v; }
    void sync_ref() { ref = (fmark[0] == 1 && fmark[1] == 1) ? 1 : (fmark[0] == 2 && fmark[1] == 2) ? 2 : (fmark[0] || fmark[1]) ? 3 : 0; }
    bool any_short() const { return fmark[0] == 1 || fmark[1] == 1; }
    bool any_long() const { return fmark[0] == 2 || fmark[1] == 2; }
    bool wait_output = false;
    int poc = 0, frame_num = 0, frame_num_wrap = 0, pic_num = 0, lt_idx = -1;
    int decode_idx = 0; bool mmco5 = false;
    std::shared_ptr<MotionField> mf;           // motion of the FRAME picture (colocated data of later B frames)
    std::shared_ptr<MotionField> mf_fld[2];    // ... of the field pictures that filled the store (colocated data of later B fields)
    std::shared_ptr<HevcColMotion> hcol;       // HEVC: motion of this picture for temporal prediction
    int out_at = -100;                         // decode index of the picture after which this surface was displayed (cooling)
};

struct SliceTask {
    SliceHeader sh;
    std::vector<uint8_t> rbsp;                 // unescaped NAL payload (+ slack)
    size_t rbsp_len = 0;
    SliceRefs refs;
    std::shared_ptr<MotionField> col;          // keeps RefPicList1[0]'s motion field alive (B slices)
    SliceWp wp; bool has_wp = false;           // weighted prediction tables of this slice
};

// HEVC picture: the slice segments with their reference lists, and where the packed job lists sit in the job buffer
struct HevcSliceTask { HevcSliceHeader sh; HevcSliceRefs refs; std::vector<uint8_t> rbsp; size_t len = 0; };
struct HevcTask {
    HevcSps sps; HevcPps pps; int poc = 0, work_slot = -1;
    std::vector<HevcSliceTask> slices;
    std::shared_ptr<HevcColMotion> col_out;
    size_t off_ctbs = 0, off_qp8 = 0, off_pus = 0, off_tbs = 0, off_itbs = 0, off_coefs = 0, off_wps = 0;
    int n_pus = 0, n_tbs = 0, n_itbs = 0; bool any_sao = false, any_deblock = false;
    HevcPicHash hash;                          // option verify_hash: what the picture's suffix SEI says its samples hash to (type -1: nothing)
};

// MJPEG picture (codec_type 2): its headers' snapshot, its entropy-coded bytes, and where the packed job list sits in the job buffer
// on_device: option jpeg_device_entropy sends the picture's scan to k_jpeg_entropy -- the job buffer then holds tables, segment table and clean bytes
// (off_tab, off_segs, off_bytes), and off_first / off_count / off_entries are offsets into the slot's device-only buffer; host_error: the
// segmenter has already counted the picture in `errors`
struct JpegTask { JpegPic pic; std::vector<uint8_t> data; size_t off_first = 0, off_count = 0, off_entries = 0; int n_entries = 0;
    bool on_device = false, host_error = false; size_t off_tab = 0, off_segs = 0, off_bytes = 0; int n_segs = 0; };

// MPEG-2 picture (codec_type 4): its headers' snapshot with the slices' bytes, the reference surfaces, and where the job list sits in the job buffer
// on_device: option mpeg2_device_vlc sends the picture's slices to k_mpeg2_vlc -- the job buffer then holds the picture's VLC parameters, the slice
// table and the slice bytes (off_par, off_slices, off_bytes), and off_mbs / off_entries are offsets into the slot's device-only buffer
// option mpeg2_field_pictures: structure 1 / 2 = a top / bottom field picture, decoded into the lines of that parity of cur_slot; fref_slot /
// fref_par: per direction and parity the surface and the lines (parity) of the reference field, -1 = none.  fill: no coded picture -- the missing
// field of a lone first field of an anchor, written as zero-vector copies of the field that exists (fref names it for both parities), so that
// later pictures find a whole frame.  ext: the records need the kernel instantiation with the field-picture modes (set by the parse worker)
struct Mpeg2Task { Mpeg2Pic pic; int ref_slot[2] = {-1, -1}; size_t off_mbs = 0, off_entries = 0; int n_entries = 0;
    bool on_device = false; size_t off_par = 0, off_slices = 0, off_bytes = 0; int n_slices = 0;
    int structure = 0; int fref_slot[2][2] = {{-1, -1}, {-1, -1}}, fref_par[2][2] = {{0, 1}, {0, 1}}; bool fill = false, ext = false; };

// VP8 key frame (codec_type 5): the frame's bytes and what its first ten say; the parse worker fills in the rest of the header and where the job list
// (records, entries: vp8_jobs.h) sits in the job buffer
struct Vp8Task { Vp8FrameTag tag; std::vector<uint8_t> data; bool truncated = false; size_t off_mbs = 0, off_entries = 0; int n_entries = 0;
    int filter_type = 0, sharpness = 0; bool filtered = false; int16_t dq[4][6] = {{0}};
    // option vp8_inter: an inter frame's reference surfaces (last, golden, altref; chosen by the caller thread), and what the parse adds
    int ref_slot[3] = {-1, -1, -1}; bool inter = false; int interp = 0, n_intra = 0, n_split = 0, n_inter = 0; size_t off_split = 0; };

struct PicTask {
    uint64_t seq = 0;
    bool has_picture = false;
    int cur_slot = -1, job_slot = -1;
    int field = 0;                             // 0 frame picture, 1 / 2 top / bottom field picture (sps.mb_h is then the FIELD's)
    std::shared_ptr<MotionField> mf;           // this picture's motion field (reference pictures of streams that may hold B pictures)
    SeqParams sps; PicParamSet pps;
    std::vector<SliceTask> slices;
    std::unique_ptr<HevcTask> hevc;            // codec_type 1
    std::unique_ptr<JpegTask> jpeg;            // codec_type 2
    std::unique_ptr<Mpeg2Task> mpeg2;          // codec_type 4
    std::unique_ptr<Vp8Task> vp8;              // codec_type 5
    std::vector<int> out_before, out_after;    // frames to display before / after this picture (Decoder::display_entry)
    bool wait_prev_pack = false;               // current surface was displayed by the previous picture (no cooling slack)
    // written by the parse worker
    std::atomic<int> state{0};                 // 0 queued, 1 parsed
    int n_intra = 0, n_i8x8 = 0, n_slices = 0; bool any_deblock = false;
    uint32_t coef_count = 0, mv_ext_count = 0; size_t upload_bytes = 0, wp_offset = 0; bool any_wp = false;
    int max_mvy = 0, max_mvx = 0;              // largest downward / rightward vector component (quarter samples): spacing of chain launches
    unsigned long long upload_seq = 0;
    std::string error;
    long long t_dispatch = 0, t_parsed = 0;    // host steady-clock ns (JM_AMD_DEC_TRACE)
};

struct JobSlot {                       // one picture's job list: pinned host buffer (parse target) + its device copy
    uint8_t *host = nullptr, *dev = nullptr; size_t cap = 0;
    // device scratch: int16 residual of this picture's intra macroblocks (768 B per macroblock), per slot for the same reason
    uint8_t *resid = nullptr;
    // device scratch of k_deblock_prep for this picture (96 B per macroblock): per slot, because pictures of a chain run concurrently
    uint8_t *dbrec = nullptr;
    ihipEvent_t *uploaded = nullptr;   // recorded behind the H2D copy on the engine's copy stream
    // MJPEG, option jpeg_device_entropy: what only the device reads and writes (first / count / entries of k_jpeg_entropy): device memory with no
    // page-locked mirror, grown on demand (Decoder::ensure_dev_only); a parse-only handle records the size and allocates nothing.  MPEG-2, option
    // mpeg2_device_vlc: the records and entries of k_mpeg2_vlc likewise
    uint8_t *dev_only = nullptr; size_t dev_only_cap = 0;
    bool busy = false;                 // from dispatch until the engine reports the picture done
    int big = -1;                      // >= 0: host / dev / cap are those of borrowed big buffer `big` (an I picture); the slot's own are kept below
    uint8_t *own_host = nullptr, *own_dev = nullptr; size_t own_cap = 0;
};
// HEVC pictures of one handle that may share a batch (independent B pictures of a pyramid): each needs its own pre-SAO work surface and residual scratch
constexpr int kHevcWorkSets = 4;
// worst-case-sized job buffers per H.264 handle, lent to I pictures (one in thirty pictures of config C1; two in flight at most)
constexpr int kBigJobBufs = 3;
struct BigJobBuf { uint8_t *host = nullptr, *dev = nullptr; bool busy = false; };
struct OutSlot {                       // one display frame in pinned host memory, written by k_packout
    uint8_t *host = nullptr;
    uint8_t *dev = nullptr;            // device staging of the packed frame (copy-engine mode, see Engine::launch)
    size_t bytes = 0;
    int w = 0, h = 0;                  // display size of the frame held (a stream may change resolution at an IDR picture)
    size_t fbytes = 0;                 // bytes of the frame held (w * h * 3 / 2, or the RGB frame's)
    bool has_data = false, ready = false;
    bool fetch = false;                // this frame waits in device staging and jm_nvdec_output_frame copies it with one synchronous DMA (Decoder::init)
};

class HostCopier;

// Scaled / cropped output: build_scale_taps (scale_packed.h) makes the tap table of one axis of the resampler R_G;
// the four tables of a geometry (crop w x h -> target tw x th: luma x, luma y, chroma x, chroma y) in ONE device allocation *dev (the caller
// frees it); ax[] points into it.  Synchronous (activation time).  false: invalid sizes or a failed allocation.
bool upload_scale_tables(int w, int h, int tw, int th, uint8_t **dev, ScaleAxis ax[4]);
// Placed output (INTEGRATION.md "Placed output"): the letterbox rectangle of a cw x ch picture with sample aspect ratio sar_num : sar_den (a zero term:
// square samples) inside a tw x th target; fit 1 centred, 2 at the top left.  rect = x, y, w, h, all even.  false: invalid arguments.
bool fit_rect(int cw, int ch, int sar_num, int sar_den, int tw, int th, int fit, int rect[4]);

// RGB output (INTEGRATION.md "RGB output"): the spec of jm_amddec_set_rgb (same layout as jm_amddec_rgb_spec)
struct RgbSpec { int dtype, planar, bgr, matrix, range; float scale[3], bias[3]; };
bool rgb_spec_valid(const RgbSpec &s, bool need_matrix);
// the chroma x / y tables of crop w x h -> the full target tw x th at chroma_sample_loc_type loc (build_chroma_taps, chroma_packed.h), uploaded
bool upload_chroma_tables(int w, int h, int tw, int th, int loc, uint8_t **dev, ScaleAxis cax[2]);
inline int rgb_sample_bytes(int dtype) { return dtype == RGB_U8 ? 1 : (dtype == RGB_F32 ? 4 : 2); }
// cy, crv, cgu, cgv, cbu of H.273 MatrixCoefficients `matrix` (1, 4, 5, 6, 7, 9), limited or full range; false when unsupported
bool color_coefs(int matrix, bool full_range, int c[5]);
// the colour part of an RgbJob (coefficients, offset, sample type, layout, k / b) for a resolved matrix and range
bool fill_rgb_color(RgbJob &j, const RgbSpec &s, int matrix, bool full_range);

class Decoder {
public:
    Decoder();
    ~Decoder();
    int  init(int codec_type, int out_fmt, const uint8_t *extra, int len);
    int  decode(const uint8_t *buf, int len, int *got_frame);
    int  poll(int *got_frame, int wait_us = 0); // pop a finished display frame without feeding input (wait_us > 0: wait that long for one that is on its way)
    int  push(const uint8_t *buf, int len);    // feed input without popping a frame (the current frame stays current)
    int  push_eos();                           // end of stream without popping a frame
    int  output(uint8_t *out, int *out_len);
    int  output_device(void **dev, int *len);
    int  output_argb_device(void *dev_dst, int pitch);
    int  output_nv12_pitch_device(void *dev_dst, int pitch);
    int  stream_info(int *w, int *h) const;
    void set_eof(bool e) { eof_flag_ = e; }
    bool is_exit() const { return is_exit_; }
    bool field_rate() const { return deint_mode_ && deint_rate_; }     // options deinterlace + deinterlace_rate: a picture may leave as two frames
    char *info() { return info_; }
    const char *last_error();
    int codec() const { return codec_; }
    // a call this codec does not offer: the reason is left for last_error(), the handle goes on
    void refuse_call(const std::string &msg) { note_error(msg); }
    int  set_option(const char *key, long long v);
    int  set_rgb(const RgbSpec *spec);         // before init; nullptr = Y'CbCr output again
    long long get_stat(const char *key) const;
    void set_device(int d) { device_ = d; }
    int  numa_node() const { return numa_node_; }   // NUMA node of this handle's GPU (-1: unknown / one-node host): which parse pool it uses
    void api_exception(const char *what) { fail(std::string("exception in the decoder: ") + what); }
    void parse_exception(PicTask *t, const char *what);   // worker-pool: an exception escaped parse_task

    // worker-pool entry
    void parse_task(PicTask *t, ParseScratch &scratch);
    // engine completion callback + engine-private per-decoder state
    void on_engine_done(const struct EnginePic &p, bool failed = false);
    void on_engine_error(const std::string &msg) { fail(msg); }     // engine: a resource this handle's frames need could not be had
    void on_device_wait_error(int code);       // engine: a kernel's bounded wait gave up while this handle's picture was decoded
    // engine: the device's hashes of a picture that carried a CRC / checksum SEI (words: CRC of Y, Cb, Cr, then their checksums; nullptr = the picture's
    // batch failed or was recovered, nothing to compare); bad: -1, or the first component whose value differs from the SEI's
    void on_picture_hash(const struct EnginePic &p, const uint32_t *words, int bad);
    // ... and of a picture that carried an MD5 SEI (option verify_md5): digests = 3 x 16 bytes, Y, Cb, Cr; bad as above
    void on_picture_md5(const struct EnginePic &p, const uint8_t *digests, int bad);
    // engine: the status words k_jpeg_entropy left for a device-path MJPEG picture (damaged segments, kinds of damage: jpeg_jobs.h)
    void on_jpeg_entropy_status(const struct EnginePic &p, uint32_t damaged, uint32_t kinds);
    // engine: the kMpeg2StatusWords status words k_mpeg2_vlc left for a device-path MPEG-2 picture (mpeg2_jobs.h)
    void mpeg2_device_status(const struct EnginePic &p, const uint32_t *words);
    struct EngineDecoderState &engine_state() { return *eng_state_; }
    // display frames that are decoded and packed and that the caller has not fetched yet (the engine asks: is this handle's next picture urgent?)
    int frames_done_unfetched() const { return done_unfetched_.load(std::memory_order_relaxed); }

private:
    // ---- front end (caller thread) ----
    void feed(const uint8_t *buf, size_t len);
    void flush_stream();
    void handle_nal(const uint8_t *nal, size_t len);
    bool start_picture(const SliceHeader &sh, const SeqParams &sps, const PicParamSet &pps);
    void add_slice(const SliceHeader &sh, std::vector<uint8_t> &&rbsp, size_t rbsp_len);
    void dispatch_pending();
    void build_ref_lists(const SliceHeader &sh, SliceTask &st);
    void mark_current(const SliceHeader &sh);
    int  compute_poc(const SliceHeader &sh, DpbPic &store);
    void build_field_ref_lists(const SliceHeader &sh, SliceTask &task);
    void build_frame_ref_lists(const SliceHeader &sh, SliceTask &task);
    void mark_current_field(const SliceHeader &sh);
    void store_done(int slot, std::vector<int> &out);
    // a display frame as the engine gets it: slot | lone field << 8 | colour << 16 | kept field << 24 (DpbPic::lone, DpbPic::color, the
    // deinterlacer's decision: 0 = not deinterlaced, 1 top, 2 bottom), taken when the frame is queued; bit 26: a field-rate pair; bits 27..31: 1 + the
    // slot of the previous display frame when D reads it (option deinterlace_temporal), 0 = none
    int  display_entry(int slot);
    void infer_frame(int frame_num);
    void bump_after_current(std::vector<int> &out);
    void flush_dpb(std::vector<int> &out);
    void push_task(std::unique_ptr<PicTask> t);
    bool activate(const SeqParams &sps);
    int  acquire_job_slot(bool big = false);
    int  pop_output(bool block, int wait_us = 0);
    void fail(const std::string &msg);
    void note_error(const std::string &msg);
    // ---- device side ----
    bool gpu_open();
    bool gpu_alloc_sequence();
    void gpu_free_sequence();
    void free_out_slots(bool all);
    // ---- HEVC front end (hevc_decoder.cpp) ----
    void hevc_handle_nal(const uint8_t *nal, size_t len);
    bool hevc_start_picture(const HevcSliceHeader &sh, int nal_type, int tid);
    bool hevc_activate(const HevcSps &sps);
    bool hevc_build_refs(const HevcSliceHeader &sh, HevcSliceRefs &refs);
    void hevc_dispatch_pending();
    void hevc_handle_suffix_sei(const uint8_t *nal, size_t len);
    void hevc_bump(std::vector<int> &out, bool all, bool use_fullness);
    void hevc_parse_task(PicTask *t);
    void hevc_fill_engine_pic(PicTask *t, struct EnginePic &ep);
    bool ensure_job_cap(JobSlot &js, size_t bytes, size_t keep = 0);
    bool ensure_dev_only(JobSlot &js, size_t bytes);      // (jpeg_decoder.cpp)
    // ---- MJPEG front end (jpeg_decoder.cpp) ----
    void jpeg_feed(const uint8_t *buf, size_t len);
    void jpeg_flush();
    void jpeg_handle_picture(const uint8_t *p, size_t n, bool truncated);
    bool jpeg_activate(const JpegPic &pic);
    void jpeg_parse_task(PicTask *t);
    void jpeg_parse_task_device(PicTask *t);   // option jpeg_device_entropy: the segmenter instead of the Huffman decode
    void jpeg_fill_engine_pic(PicTask *t, struct EnginePic &ep);
    // ---- MPEG-2 front end (mpeg2_decoder.cpp) ----
    void mpeg2_feed(const uint8_t *buf, size_t len);
    void mpeg2_flush();
    void mpeg2_after_split();
    void mpeg2_handle_picture(Mpeg2Pic &pic);
    bool mpeg2_activate(const Mpeg2Seq &seq);
    void mpeg2_show_anchor(std::vector<int> &out);
    void mpeg2_close_pending();                // option mpeg2_field_pictures: the waiting first field stays a lone field
    void mpeg2_parse_task(PicTask *t);
    bool mpeg2_parse_task_device(PicTask *t);  // option mpeg2_device_vlc: the prescan instead of the VLC decode; false: the host path takes the picture
    void mpeg2_fill_engine_pic(PicTask *t, struct EnginePic &ep);
    // ---- VP8 front end (vp8_decoder.cpp) ----
    void vp8_feed(const uint8_t *buf, size_t len);
    void vp8_flush();
    void vp8_handle_frame(const uint8_t *p, size_t n, bool truncated);
    bool vp8_activate(const Vp8FrameTag &tag);
    void vp8_parse_task(PicTask *t);
    void vp8_update_refs(const Vp8Pic &pic, int cur);      // option vp8_inter
    void vp8_fill_engine_pic(PicTask *t, struct EnginePic &ep);
    void gpu_close();
    void submit_ready();
    void submit_task(PicTask *t);
    void enqueue_output(int entry, OutSide &out);
    bool resolve_geometry();                   // options crop_* / target_* against the display size of the sequence being activated
    // the colour description of the sequence being activated (vui: full range, primaries, transfer, matrix as transmitted, -1 = absent): the
    // matrix and range its frames are converted with
    void resolve_color(const int vui[4], int disp_h);
    // the chroma sample location of the sequence being activated (the VUI's top / bottom values as transmitted, -1 = absent; fallback: what the codec
    // implies without one -- 0 for H.264 / HEVC, 1 for JFIF).  true: the location in use changed and the handle interpolates chroma (new tap tables)
    bool resolve_chroma_loc(int vui_top, int vui_bottom, int fallback);
    OutSlot *alloc_out_slot();

    // configuration
    int codec_ = 0, out_fmt_ = 1, device_ = -1, handle_index_ = 0, last_surf_ = -1, out_route_ = 0, fetch_limit_ = 1;
    bool chain_ok_ = false, chain_intra_on_ = true;
    bool parse_only_ = false, want_digest_ = false, sync_mode_ = false, profile_ = false, out_via_copy_engine_ = true, device_output_ = false,
        out_fetch_ = true;
    std::string error_, error_out_; std::mutex error_m_;     // error_out_: what last_error() last handed out (see there)
    std::atomic<bool> failed_{false}; bool inited_ = false;

    // splitter
    std::vector<uint8_t> in_; size_t scan_ = 0; bool have_start_ = false; size_t nal_start_ = 0;
    int avcc_len_size_ = 0;                    // > 0: init got an avcC record; packets are length-prefixed NAL units of this many bytes

    // parameter sets / sequence
    ParamSets ps_;
    bool seq_active_ = false; SeqParams seq_;
    int mb_w_ = 0, mb_h_ = 0, disp_w_ = 0, disp_h_ = 0, dpb_size_ = 1, reorder_depth_ = 0, n_surf_ = 0;
    // scaled / cropped output (options before init): crop x, y, w, h (w / h 0: to the display area's edge), target w, h (0: the crop size)
    int geo_[6] = {0, 0, 0, 0, 0, 0};
    // ... resolved per sequence (resolve_geometry): the size of the frames handed out, the crop rectangle; scaled_ = not the identity
    int out_w_ = 0, out_h_ = 0, crop_[4] = {0, 0, 0, 0}; bool scaled_ = false;
    uint8_t *scale_dev_ = nullptr; ScaleAxis scale_ax_[4] = {};     // the sequence's tap tables on the device (k_scale_pack)
    // placed output (options before init): rect_x, rect_y, rect_w, rect_h (w / h 0: to the target's edge), fit, fit_sar, fill (-1: the default colour)
    int rect_opt_[4] = {0, 0, 0, 0}, fit_ = 0, fit_sar_ = 0; long long fill_ = -1;
    // ... resolved per sequence (resolve_geometry): the picture's rectangle inside the target; placed_ = it is not the whole target (then scaled_ is set
    // and the tap tables are those of crop -> rectangle); rgb_identity_: k_rgb_pack reads the surface directly
    int place_[4] = {0, 0, 0, 0}; bool placed_ = false, rgb_identity_ = false;
    int sar_[2] = {0, 0};                      // the active sequence's sample aspect ratio as transmitted, 0 : 0 = absent
    std::atomic<long long> stat_placed_{0};
    std::atomic<long long> stat_scaled_{0};
    // RGB output (jm_amddec_set_rgb, before init): every display frame leaves as C(R_G(F)) through k_rgb_pack
    bool rgb_ = false; RgbSpec rgb_spec_ = {};
    int vui_[4] = {-1, -1, -1, -1};            // the active sequence's VUI: full range, primaries, transfer, matrix (-1 = absent)
    int color_matrix_ = 0, color_range_ = 0;   // ... resolved (resolve_color): H.273 matrix, 1 limited / 2 full
    std::atomic<long long> stat_rgb_{0};
    // interpolated chroma (options rgb_chroma, chroma_loc, before init): C is applied to the 4:4:4 frame G' through k_rgb_pack444 (chroma_packed.h)
    int rgb_chroma_ = 0, chroma_loc_opt_ = -1;                      // chroma_loc_opt_: -1 auto, 0..5 forced
    int vui_chroma_loc_[2] = {-1, -1}, chroma_loc_ = 0;             // the active sequence's VUI values (top, bottom); the location in use (frame siting)
    uint8_t *chroma_dev_ = nullptr; ScaleAxis chroma_ax_[2] = {};   // the sequence's chroma x / y tables to the full target, on the device
    std::atomic<long long> stat_rgb_chroma_{0};
    // deinterlaced output (options deinterlace*, before init): the frames chosen by deinterlace_when leave as C(R_G(D(F))), D through k_deint
    int deint_mode_ = 0, deint_when_ = 0, deint_field_ = 0, deint_thr_ = 0;      // (deint_thr_: T, 0 = 10)
    int deint_rate_ = 0;                       // option deinterlace_rate: 1 = field rate, a frame chosen for D leaves as D_f(F), D_f'(F) (k_deint2)
    std::atomic<long long> stat_deint_{0}, stat_pairs_{0};
    // motion-adaptive deinterlacing (option deinterlace_temporal, acts while deinterlace is 2): a frame chosen for D leaves as D3(F, F') -- k_deint3 -- when
    // the display picture before it, F', was chosen for D too, neither is a lone field and both belong to this activation.  F' is kept by holding its
    // SURFACE: hold_ is the slot of the last display picture chosen for D; it is not handed to a new picture (slot_free) until the next display picture
    // has been queued (display_entry), whose task names it in its out_mask -- the engine orders every writer of a surface behind those readers.
    int deint_temporal_ = 0, hold_ = -1;
    bool temporal() const { return deint_temporal_ && deint_mode_ == 2; }
    bool slot_free(int i) const { return !dpb_[i].in_use && i != hold_; }
    std::atomic<long long> stat_temporal_{0};

    // DPB / picture state (front end only)
    DpbPic dpb_[kMaxSurfaces];
    int cur_ = -1;
    int cur_field_ = 0; bool cur_second_ = false;   // the current picture: 0 frame, 1 top field, 2 bottom field; the second field of its frame
    int prev_ref_frame_num_ = 0;                    // PrevRefFrameNum (7.4.3)
    std::atomic<long long> stat_inferred_frames_{0}, stat_redundant_slices_{0};
    int pending_first_ = -1;                        // the frame store that holds a first field and waits for the second
    std::atomic<long long> stat_field_pics_{0}, stat_lone_fields_{0};
    std::unique_ptr<PicTask> pending_;
    SliceHeader first_sh_;
    int prev_poc_msb_ = 0, prev_poc_lsb_ = 0, prev_frame_num_ = 0; long long prev_frame_num_offset_ = 0; bool prev_mmco5_ = false;
    int numa_node_ = -1;
    long long cur_top_poc_ = 0, cur_bot_poc_ = 0;   // TopFieldOrderCnt / BottomFieldOrderCnt of the current picture (pic_order_cnt_type 0)
    int decode_count_ = 0, max_lt_idx_ = -1;
    uint64_t next_seq_ = 0;
    std::vector<int> carry_out_;               // outputs decided before the next picture starts (IDR flush)

    // task pipeline
    std::mutex mtx_;                           // guards inflight_, job slots, out queue
    std::condition_variable cv_;
    std::deque<std::unique_ptr<PicTask>> inflight_;
    std::mutex submit_mtx_;
    JobSlot jobs_[kMaxJobSlots]; int n_jobs_ = kJobSlots;      // the first n_jobs_ are in use (option "job_slots", before init)
    bool n_jobs_set_ = false;                                  // ... chosen by the caller; else by picture size (gpu_alloc_sequence)
    BigJobBuf big_[kBigJobBufs];               // see acquire_job_slot
    void free_job_buffers();
    std::deque<OutSlot *> ready_;              // display order
    std::atomic<int> done_unfetched_{0};       // entries of ready_ whose samples are there (OutSlot::ready)
    std::vector<OutSlot *> free_out_, all_out_;
    OutSlot *cur_out_ = nullptr;
    int outstanding_ = 0, parse_pending_ = 0;                      // tasks pushed and not yet submitted

    // device
    struct EngineDecoderState *eng_state_ = nullptr;
    class Engine *engine_ = nullptr;          // per-device executor (engine.h): the only place device work is issued
    uint8_t *surf_[kMaxSurfaces] = {nullptr};
    uint8_t *surf_block_ = nullptr;            // ONE device allocation holds every surface (surf_[i] = block + i * stride): the chain kernels address all of
                                               // a picture's references through one buffer descriptor (recon_device.h RefBuf)
    void free_surfaces();
    bool use_lds_deblock_ = false;
    uint8_t *resid_ = nullptr; bool use_lds_intra_ = false; bool lds_intra8_ = false;
    // HEVC: pre-SAO work surfaces (resid_ holds as many residual scratches)
    uint8_t *hevc_work_[kHevcWorkSets] = {nullptr, nullptr, nullptr, nullptr}; unsigned hevc_work_rr_ = 0;
    // HEVC boundary strengths on the device (round 5): per work set the 4x4-cell maps and the strength arrays (hevc_jobs.h HevcPicParams)
    uint8_t *hevc_bs_ = nullptr; size_t hevc_bs_set_bytes_ = 0, hevc_bs_off_[4] = {0, 0, 0, 0};
    int pitch_ = 0, chroma_off_ = 0; size_t surf_bytes_ = 0, frame_bytes_ = 0, job_cap_ = 0, job_cap_max_ = 0;
    std::atomic<size_t> i_job_peak_{0};            // largest job list of an I picture of this handle so far (+ slack): what a slot grows to for the next one
    std::atomic<long long> stat_job_regrown_{0};   // job slots grown (a few per handle while the slots reach their working size)
    bool gpu_open_ = false;

    // status / stats
    bool eof_flag_ = false, is_exit_ = false;
    std::atomic<bool> eos_sent_{false};        // (set by the thread that feeds, read by the thread that takes frames: jm_amddec_push_eos)
    uint32_t num_frames_ = 0;
    std::chrono::steady_clock::time_point t0_; bool timer_started_ = false; double elapsed_ms_ = 0;
    char info_[1024];
    std::atomic<long long> stat_parse_ns_i_{0}, stat_parse_ns_p_{0}, stat_submit_ns_{0}, stat_wait_slot_ns_{0};
    std::atomic<long long> stat_pictures_{0}, stat_job_bytes_{0}, stat_errors_{0}, stat_intra_mbs_{0}, stat_coef_{0}, stat_wait_errors_{0};
    SyntaxDigest digest_;
    bool fast_parse_ = true, want_job_digest_ = false;
    // output route "direct" (host_copy.h)
    std::atomic<long long> stat_direct_{0}, stat_direct_ns_{0};
    HostCopier *copier_ = nullptr; uint64_t out_sig_ = 0;
    // a frame goes out only while this many pictures of the handle are still on their way (option "display_delay", JM_AMD_DEC_DISPLAY_DELAY)
    int display_delay_ = 0;
    uint64_t job_digest_ = 1469598103934665603ull;    // option "job_digest" (tests)
    // HEVC state (front end only unless noted)
    HevcParamSets hps_; HevcSps hsps_; HevcPps hpps_;
    int h_poc_tid0_ = 0, h_max_dpb_ = 1, h_reorder_ = 0, extra_surf_ = 0; bool h_first_picture_ = true, h_no_rasl_output_ = false, h_seen_eos_ = false;
    HevcSliceHeader h_last_sh_; bool h_have_last_sh_ = false;
    HevcDigest hdigest_;                       // written by the parse worker (sync option)
    long long stat_i_ = 0, stat_p_ = 0, stat_b_ = 0;
    std::vector<int> display_pocs_;            // diagnostic (get via stats)
    // option verify_hash (before init): 0 off -- suffix SEI is not looked at; 1 verify and count; 2 a mismatch fails the handle
    int verify_hash_ = 0;
    int verify_md5_ = 0;                       // option verify_md5 (before init): 1 = MD5 messages are compared too (only with verify_hash 1 or 2)
    std::atomic<uint32_t> hash_last_md5_[12] = {};      // the device's digests of the most recent MD5-verified picture: per component four big-endian words
    std::atomic<long long> stat_hash_pics_{0}, stat_hash_checked_{0}, stat_hash_mismatch_{0}, stat_hash_unchecked_{0}, stat_hash_md5_{0};
    std::atomic<long long> stat_hash_bad_poc_{-2147483648ll};
    std::atomic<uint32_t> hash_last_[6] = {};  // the device's words of the most recently completed hashed picture (engine thread writes)
    struct HashSeen { int poc; HevcPicHash h; };
    std::vector<HashSeen> hash_seen_;          // diagnostic (stats hash_sei_*): the hash messages in decode order, the first 65536
    std::vector<uint8_t> display_fields_;      // per output frame: the kept field (display_entry); only filled with option deinterlace
    std::vector<uint8_t> display_temporal_;    // per output frame: 1 = its D read the previous display frame (display_entry); only filled with option deinterlace
    std::vector<uint32_t> display_pics_;       // per output frame: the display picture it shows (display_entry); only filled at field rate
    uint32_t display_count_ = 0;               // display pictures queued so far (display_entry calls)
    // MJPEG state (front end only unless noted)
    JpegSplitter jsplit_; JpegTables jtab_;
    int j_w_ = 0, j_h_ = 0, j_sampling_ = 0; unsigned j_surf_rr_ = 0;
    std::atomic<long long> stat_jpeg_pics_{0}, stat_jpeg_ri_{0};
    // option jpeg_device_entropy (before init): 0 host Huffman decode; 1 pictures with a restart interval and at least 2 segments are entropy-decoded
    // by k_jpeg_entropy; 2 every picture is
    int jpeg_dev_entropy_ = 0;
    std::atomic<long long> stat_jpeg_dev_pics_{0}, stat_jpeg_host_pics_{0}, stat_jpeg_dev_segs_{0}, stat_jpeg_dev_damaged_{0};
    // MPEG-2 state (front end only unless noted)
    Mpeg2Splitter m2split_; Mpeg2Seq m2seq_; long long m2_damaged_seen_ = 0;
    int m2_anchor_[2] = {-1, -1};              // surfaces of the older / newer anchor picture (-1: none)
    bool m2_anchor_shown_ = true;              // the newer anchor has been queued for display (it waits for the next anchor, or the flush)
    std::atomic<long long> stat_dropped_{0}, stat_m2_clamped_{0}, stat_m2_rff_{0};
    // option mpeg2_device_vlc (before init): 1 = pictures are VLC-decoded by k_mpeg2_vlc, one lane per slice, unless the prescan sends them to the host path
    int mpeg2_dev_vlc_ = 0;
    // option mpeg2_field_pictures (before init): 1 = field pictures, 16x8 motion compensation and dual prime are decoded; 0 = they fail the handle
    int mpeg2_field_pics_ = 0;
    int m2_pend_slot_ = -1, m2_pend_par_ = 0, m2_pend_type_ = 0;      // the frame whose first field picture waits for its second: surface, parity, type
    std::atomic<long long> stat_m2_fields_{0}, stat_m2_lone_{0}, stat_m2_dual_{0}, stat_m2_16x8_{0};
    std::atomic<long long> stat_m2_dev_pics_{0}, stat_m2_host_pics_{0}, stat_m2_dev_slices_{0}, stat_m2_dev_damaged_{0};
    uint64_t m2_digest_ = 1469598103934665603ull; long long m2_digest_mbs_ = 0;      // written by the parse worker (sync option)
    // VP8 state (front end only unless noted)
    int vp8_on_ = 0;                           // option vp8 (before init): 1 = init accepts codec_type 5
    Vp8Splitter v8split_; int v8_w_ = 0, v8_h_ = 0; long long v8_key_seen_ = 0;
    // option vp8_inter (before init): 1 = inter frames are decoded; 0 = they fail the handle ("VP8 inter frames are not built").  With it a stream's
    // frames are parsed in order on the caller thread (frame n + 1 reads the probabilities, the segment map and the deltas frame n left: v8_state_),
    // and last / golden / altref are slots of the surface pool (v8_ref_; -1 before the first key frame) that the round robin skips
    int vp8_inter_ = 0; Vp8State v8_state_; int v8_ref_[3] = {-1, -1, -1};
    std::atomic<long long> stat_v8_inter_{0}, stat_v8_golden_{0}, stat_v8_altref_{0}, stat_v8_split_{0}, stat_v8_intra_in_inter_{0};
    // (the last five describe the last picture parsed, written by the parse worker: read them after the handle has drained, or with option sync)
    std::atomic<long long> stat_v8_key_{0}, stat_v8_hidden_{0}, stat_v8_empty_{0}, stat_v8_bpred_{0}, stat_v8_skipped_{0};
    std::atomic<int> stat_v8_parts_{0}, stat_v8_segments_{0}, stat_v8_filter_{0}, stat_v8_color_{0}, stat_v8_scale_{0};
    struct TraceRec { uint64_t seq; long long t_dispatch, t_parsed, t_submit0, t_submit1; int is_i; };
    std::vector<TraceRec> trace_; bool trace_on_ = false;
};

// process-wide parse worker pool
void pool_submit(Decoder *d, PicTask *t);
int  pool_threads(int numa_node);

}  // namespace jmamd
