/*
 * include/jm_amd_dec.h -- C ABI of the MI355X-native decode backend (libjm_amd_dec.so).
 *
 * Every entry point mirrors one function of the reference's public decode API
 * (/root/reference/nv_dec/jm_nv_dec.h) 1:1 -- same argument order, meaning and
 * return conventions -- with plain C types so that any FFI can bind it.  The
 * same library ALSO exports the reference's own C++-mangled jm_nvdec_* symbols
 * (jmcodec_amd/csrc/jm_nv_dec_api.cpp) so that test_nv_dec.cpp links unchanged.
 *
 *   jm_amddec_create_handle   <- jm_nvdec_create_handle   jm_nv_dec.h:27   (nv_dec.cpp:695-698)
 *   jm_amddec_init            <- jm_nvdec_init            jm_nv_dec.h:39   (nv_dec.cpp:710-713)
 *   jm_amddec_deinit          <- jm_nvdec_deinit          jm_nv_dec.h:47   (nv_dec.cpp:721-724)
 *   jm_amddec_decode_frame    <- jm_nvdec_decode_frame    jm_nv_dec.h:58   (nv_dec.cpp:735-739)
 *   jm_amddec_output_frame    <- jm_nvdec_output_frame    jm_nv_dec.h:68   (nv_dec.cpp:750-828)
 *   jm_amddec_stream_info     <- jm_nvdec_stream_info     jm_nv_dec.h:79   (nv_dec.cpp:838-845)
 *   jm_amddec_set_eof         <- jm_nvdec_set_eof         jm_nv_dec.h:82   (nv_dec.cpp:848-851)
 *   jm_amddec_is_exit         <- jm_nvdec_is_exit         jm_nv_dec.h:84   (nv_dec.cpp:853-856)
 *   jm_amddec_show_dec_info   <- jm_nvdec_show_dec_info   jm_nv_dec.h:86   (nv_dec.cpp:858-861)
 *   jm_amddec_is_hw_support   <- jm_nvdec_is_hw_support   jm_nv_dec.h:88   (nv_dec.cpp:863-870)
 *
 * Differences from the reference, all deliberate:
 *   - init/decode_frame return -1 (and log to stderr) when no HIP device can be
 *     used or the stream is unsupported; the reference returns 0 unconditionally
 *     (nv_dec.cpp:79,493).  There is no CPU fallback.
 *   - handles are independent: N handles may be driven from N threads.
 *   - the device is chosen by JM_AMD_DEC_DEVICE, jm_amddec_set_option("device")
 *     before init, or round-robin over visible devices (reference: device 0,
 *     nv_dec.cpp:209).
 */
#ifndef JM_AMD_DEC_H
#define JM_AMD_DEC_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void *jm_amddec_handle;

jm_amddec_handle jm_amddec_create_handle(void);
/* codec_type: 0 = H.264, 1 = H.265 / HEVC Main, 2 = MJPEG, 4 = MPEG-2 video, 5 = VP8 key frames with option vp8 1 (enum nv_dec.h:37-46; the other values are refused); out_fmt: 0 = NV12, 1 = "YV12" = planar Y,U,V.
 * MJPEG: the input is any chunking of a byte stream of concatenated baseline JPEG pictures (SOI .. EOI; 4:2:0 / 4:2:2 / 4:4:4 / grey, 8 bits, one
 * interleaved Huffman scan), every picture lands in the usual NV12 surface and every output option applies; progressive, arithmetic, lossless, 12-bit,
 * CMYK and other samplings fail the handle with an error string (INTEGRATION.md "MJPEG").  extra_data is not used.  Stats: jpeg_pictures, jpeg_sampling
 * (0x22 / 0x21 / 0x11 / 0x10), jpeg_restart_intervals; with option profile k_jpeg_ns / _n / _pics / _alg_bytes.
 * Option "jpeg_device_entropy" (before init; 0 default / 1 / 2; other values and other codecs are refused): 1 = a picture whose scan has a restart interval and
 * at least 2 segments is Huffman-decoded on the device (k_jpeg_entropy, one lane per restart segment), the others on the host; 2 = every picture is (one
 * without DRI as a single segment: slow for a lone large picture).  The host then uploads the Huffman tables, a segment table and the unstuffed bytes
 * instead of the job list (layout: INTEGRATION.md "MJPEG").  Undamaged pictures decode identically; damage is contained per segment -- the rest of that
 * segment is empty, the other segments decode -- where the host path empties everything behind the damage.  Stats: jpeg_dev_pictures, jpeg_host_pictures,
 * jpeg_dev_segments, jpeg_dev_damaged_segments; with option profile k_jpeg_entropy_ns / _n / _pics / _alg_bytes.  It pays with many streams or many segments
 * per picture; a lone 1080p stream loses with one MCU row per segment and draws level from about 340 segments on (INTEGRATION.md has the figures).
 * MPEG-2: the input is any chunking of an ISO/IEC 13818-2 video elementary stream (one start-code unit per call included); frame pictures I / P / B,
 * 4:2:0, progressive and interlaced; MPEG-1, field pictures, dual prime, 4:2:2 / 4:4:4, the scalable extensions and D pictures fail the handle with
 * an error string that names the feature (INTEGRATION.md "MPEG-2").  extra_data, if given, is read as the beginning of the stream.  Stats:
 * dropped_pictures, mpeg2_clamped_mbs, mpeg2_repeat_first_field, mpeg2_profile_level; with option profile k_mpeg2_ns / _n / _pics / _alg_bytes.
 * Option "mpeg2_device_vlc" (before init; 0 default / 1; other values and other codecs are refused): 1 = the slice / macroblock / block VLC decode runs on
 * the device (k_mpeg2_vlc, one lane per slice); the host then only finds every slice's first macroblock address and uploads the picture's parameters, a
 * slice table and the slice bytes instead of the job list (layout: INTEGRATION.md "MPEG-2").  parse_only and digest handles, and pictures whose slice
 * headers the prescan cannot accept or whose slices are out of order, take the host path.  Undamaged pictures decode identically, damage is concealed by
 * the host path's rules; dual prime fails the handle when the engine reads the picture's status.  Stats: mpeg2_dev_pictures, mpeg2_host_pictures,
 * mpeg2_dev_slices, mpeg2_dev_damaged_slices; with option profile k_mpeg2_vlc_ns / _n / _pics / _alg_bytes.  When it pays: INTEGRATION.md has the figures.
 * Option "mpeg2_field_pictures" (before init; 0 default / 1; other values and other codecs are refused): 1 = field pictures (picture_structure 1 / 2;
 * I, P and B; field prediction, 16x8 motion compensation), and dual prime in P field and P frame pictures, are decoded instead of failing the handle.
 * Two field pictures of opposite parity whose types pair (I-I, I-P, P-P, B-B) make one frame in one surface; a first field whose second does not
 * follow is a lone field: its frame is displayed with the field's lines repeated (bob when deinterlacing) and `errors` increments.  display_poc and
 * `frames` count frames, i_pictures / p_pictures / b_pictures coded pictures.  With mpeg2_device_vlc as well, field pictures take the host path and
 * frame pictures stay on the device, where the lane decodes dual prime.  Stats: mpeg2_field_pictures, mpeg2_lone_fields, mpeg2_dual_prime_mbs,
 * mpeg2_16x8_mbs.  At 0 nothing changes (INTEGRATION.md "MPEG-2"). */
/* VP8 (codec_type 5): KEY frames of RFC 6386 (lossy WebP pictures, all-key-frame streams).  Option "vp8" 1 (before init) turns the codec on: without it
 * init(5) stays refused as for 3, 6 and 7, so nothing changes for a caller that does not ask (other codecs refuse the option).  The input is an IVF byte stream ("DKIF", any chunking) or one
 * whole frame per call; RIFF / WebP wrappers are not parsed.  Every key-frame feature is decoded (segmentation, both loop filters, 1-8 token partitions,
 * all quantiser deltas, B_PRED); an inter frame fails the handle with "VP8 inter frames are not built", as do a first frame that is no key frame, a bad
 * start code and sizes above 8192; deinterlace_temporal is refused at init; jm_amddec_feed_annexb is refused (no start codes).  extra_data is not
 * used.  An odd display size is handed out as the even size just above.  RGB auto: BT.601 limited range, chroma centred (INTEGRATION.md "VP8").
 * Stats: vp8_key_frames, vp8_hidden_frames, vp8_empty_frames, vp8_partitions, vp8_segments, vp8_filter_type, vp8_color_space, vp8_scale,
 * vp8_bpred_mbs, vp8_skipped_mbs; with option profile k_vp8_recon_* and k_vp8_filter_* (_ns / _n / _pics / _alg_bytes).
 * Option "vp8_inter" 1 (before init; only with codec_type 5 and "vp8" 1, init fails by name otherwise): INTER frames are decoded instead of failing the
 * handle -- last / golden / altref references with the buffer copies and sign biases of RFC 6386 9.7, ZERO / NEAREST / NEAR / NEW / SPLIT vectors, six-tap
 * (version 0) and bilinear (versions 1-3) prediction by k_vp8_inter, intra macroblocks inside inter frames, the inter-frame loop-filter deltas and
 * thresholds; probabilities, segment map and deltas are carried from frame to frame, so a stream's frames are parsed in order, on the calling thread.
 * A first frame that is no key frame stays refused.  There is NO independent decoder behind the inter-frame tests (INTEGRATION.md "VP8").  At 0 nothing
 * changes.  Stats: vp8_inter_frames (p_pictures counts them too), vp8_golden_refs, vp8_altref_refs (macroblocks predicted from them), vp8_split_mbs,
 * vp8_intra_in_inter_mbs; with option profile k_vp8_inter_*. */
int  jm_amddec_init(int codec_type, int out_fmt, char *extra_data, int len, jm_amddec_handle h);
int  jm_amddec_deinit(jm_amddec_handle h);
/* in_buf may hold any chunk of an Annex-B stream; (NULL, 0) signals end of stream and then
 * drains one display-order frame per call.  *got_frame = 1 when a frame is ready. */
int  jm_amddec_decode_frame(unsigned char *in_buf, int in_data_len, int *got_frame, jm_amddec_handle h);
/* *out_len: capacity in, bytes out.  Returns the frame size (>0), -1 no frame, -2 buffer too small. */
int  jm_amddec_output_frame(unsigned char *out_buf, int *out_len, jm_amddec_handle h);
int  jm_amddec_stream_info(int *disp_width, int *disp_height, jm_amddec_handle h);
void jm_amddec_set_eof(int is_eof, jm_amddec_handle h);
int  jm_amddec_is_exit(jm_amddec_handle h);
char *jm_amddec_show_dec_info(jm_amddec_handle h);
int  jm_amddec_is_hw_support(void);

/* ---- additions (no reference counterpart) ---- */
/* keys: "device" (before init), "device_output" (before init, see below), "sync" (1 = every call waits for the pipeline; deterministic),
 *       "parse_only" (1 = host bitstream stages only, frames carry no pixels; for host-side tests),
 *       "digest" (1 = accumulate the macroblock syntax digest; implies sync),
 *       "display_delay" (n: a frame is handed out only while n pictures of the handle are still on their way -- the reference's ulMaxDisplayDelay,
 *       nv_dec.cpp:341; default 0), "profile" (1 = time the kernels with events), "wait_idle" (block until every dispatched picture has run),
 *       engine-wide after init: "chain_depth" (pictures of one stream per chain launch; 0 = the defaults: 8, and 16 while one or two streams are active),
 *       "chain_lag", "chain_streams", "debug_stall" (DESIGN.md 4b); before init: "job_slots" (pictures in flight per handle, 8..64; default 40 for H.264 up
 *       to 1080p, else 24);
 *       "crop_x" / "crop_y" / "crop_w" / "crop_h" / "target_width" / "target_height" (before init: scaled and cropped output, see below);
 *       "verify_hash" (before init, HEVC: 1 / 2 = check the decoded picture hash SEI on the device, see below); "verify_md5" (before init, 0 / 1:
 *       with verify_hash, MD5 messages are verified too, see below);
 *       tests only: "fast_parse" (0 = every macroblock through the general parser path), "job_digest" (1 = digest of the job lists; implies sync) */
/* like jm_amddec_decode_frame without input: *got_frame = 1 when a display-order frame became ready (never signals end of stream) */
int  jm_amddec_poll_frame(int *got_frame, jm_amddec_handle h);
/* jm_amddec_poll_frame that sleeps up to timeout_us microseconds for a frame whose picture is still being decoded (returns at once when nothing is on its way) */
int  jm_amddec_wait_frame(int *got_frame, int timeout_us, jm_amddec_handle h);
/* input without taking a frame: the push half of the reference's push / pull API (intel_dec_put_input_data, /root/reference/intel_dec/intel_dec.cpp:189-234).
 * The frame signalled by an earlier got_frame = 1 stays current until the next jm_amddec_decode_frame / jm_amddec_poll_frame call.  0, or -1 on error. */
int  jm_amddec_push_data(unsigned char *in_buf, int in_data_len, jm_amddec_handle h);
/* end of stream without taking a frame (what jm_amddec_decode_frame(NULL, 0) does before it hands out a frame); drain with jm_amddec_decode_frame(NULL, 0)
 * afterwards.  jm_amddec_push_data / jm_amddec_push_eos may run on another thread than jm_amddec_poll_frame / _wait_frame / _output_frame: the facade of
 * the push / pull API feeds from a worker thread, as the reference's does (intel_dec.cpp:46-81) */
int  jm_amddec_push_eos(jm_amddec_handle h);
int  jm_amddec_set_option(jm_amddec_handle h, const char *key, long long value);
/* keys: "frames", "pictures", "job_bytes", "errors", "intra_mbs", "coef_int16", "syntax_digest",
 *       "digest_mbs", "i_pictures", "p_pictures", "coded_width", "coded_height", "pitch", "device",
 *       "threads", "elapsed_us", "failed" (1: the handle has failed, jm_amddec_last_error says why), "display_poc:<n>", "fps_num" / "fps_den" (frame rate from the VUI timing information, 0 / 0 = not transmitted),
 *       "frames_waiting" (display frames decided and not yet made current by a decode / poll call), "frames_done_unfetched" (those of them whose samples are there), "device_wait_errors", "direct_frames" / "direct_ns" (frames that left by one copy-engine
 *       transfer into the caller's buffer, and the time their callers waited), "copy_engines" (SDMA engines used for that, bit mask),
 *       "job_digest", "eng_*" / "k_*" (engine and per-kernel counters, bench.py), "out_width" / "out_height" / "scaled_frames" (see below),
 *       "hash_*" (picture hash verification, see below) */
long long jm_amddec_get_stat(jm_amddec_handle h, const char *key);
const char *jm_amddec_last_error(jm_amddec_handle h);

/* Stand-alone pack-out of one pitch-linear NV12 surface that already lives in device memory
 * (device pointers).  Same semantics as jm_nvdec_output_frame's repack (nv_dec.cpp:782-820).
 * stream: a hipStream_t or NULL.  Returns 0 or a negative hipError. */
/* SURVEY 8f f3 -- device-resident output, the path the reference stubbed out (nv_dec.h:98-107, nv_dec.cpp:244-265 under "#if 0").
 * With option "device_output" = 1 (before init) display frames are not copied to the host at all:
 *   jm_amddec_output_frame_device: *dev = device pointer of the current frame (tight NV12 / I420 as chosen at init), *len = its
 *     size; valid until the next jm_amddec_decode_frame call.  Works in the default mode too (the staging copy of the frame).
 *   jm_amddec_output_argb_device: converts the current frame to ARGB32 (memory bytes B,G,R,A; BT.601 limited range) into a device
 *     buffer of `pitch` bytes per row (>= 4 * width).  Returns 0, or -1 when no frame is current. */
int  jm_amddec_output_frame_device(void **dev, int *len, jm_amddec_handle h);
int  jm_amddec_output_argb_device(void *dev_dst, int pitch, jm_amddec_handle h);
int  jm_amddec_packout_device(const void *d_src, int pitch, int width, int height, int out_fmt,
                              void *d_dst, void *stream);
/* Scaled and cropped output (INTEGRATION.md "Scaled and cropped output" defines the resampler exactly).  Options, before init, even values only
 * (set_option returns -1 after init and for odd or negative values):
 *   "crop_x", "crop_y", "crop_w", "crop_h": the crop rectangle inside the display area (w / h 0 = up to the display area's right / bottom edge);
 *   "target_width", "target_height": the size of the frames handed out (0 = the crop size).
 * Per axis the crop may be at most 8x the target and the target at most 4x the crop.  The geometry is checked against the display area when a
 * sequence starts; a geometry that does not fit fails the handle with a jm_amddec_last_error text that says why.  stream_info, output_frame,
 * output_frame_device, output_argb_device and output_nv12_pitch_device then work on the target-size frame.  Stats: "out_width", "out_height",
 * "scaled_frames" (display frames that went through the resampler; 0 when the geometry is the identity).
 *   jm_amddec_scale_taps: the tap table of one axis, src_len -> dst_len samples (host only): first[j] = first source sample of output j (not
 *     clamped), weights[j * max_taps + k] = the weight (1/16384) of source sample clamp(first[j] + k).  Returns the taps per output, or -1 (invalid
 *     ratio, or more taps than max_taps); first == NULL or weights == NULL: only returns the taps per output.
 *   jm_amddec_scale_device: stand-alone crop + resample + pack of one pitch-linear NV12 surface in device memory (luma rows at `pitch`, the UV rows
 *     from byte chroma_offset; display area w x h; lone_field 0, or 1 / 2 = show only the top / bottom field's lines, each twice) into a tight
 *     frame of tw x th (out_fmt 0 NV12, 1 I420) at d_dst.  stream: a hipStream_t or NULL.  Returns 0, -1 for invalid arguments, or a negative
 *     hipError. */
int  jm_amddec_scale_taps(int src_len, int dst_len, int *first, short *weights, int max_taps);
int  jm_amddec_scale_device(const void *d_src, int pitch, int chroma_offset, int w, int h, int lone_field, int crop_x, int crop_y, int crop_w,
                            int crop_h, int tw, int th, int out_fmt, void *d_dst, void *stream);
/* Placed output (INTEGRATION.md "Placed output"): the resampled picture fills a rectangle inside the target, every sample outside it is a constant
 * colour; the frame handed out keeps the target size, and the one launch that writes it writes every byte once.  Options, before init (set_option
 * returns -1 after init and for odd, negative or out-of-range values):
 *   "rect_x", "rect_y", "rect_w", "rect_h": the rectangle inside the target, even values (w / h 0 = up to the target's right / bottom edge);
 *   "fit": 0 stretch (default), 1 letterbox -- the aspect ratio kept, centred --, 2 letterbox at the top left; needs both target sizes and excludes rect_*;
 *   "fit_sar": 1 = the letterbox honours the sequence's sample aspect ratio where the VUI transmits one (aspect_ratio_idc 1..16, 255);
 *   "fill": -1 (default: Y'CbCr 16, 128, 128; RGB 0, 0, 0) or 0xAABBCC = Y, Cb, Cr of a Y'CbCr handle, R, G, B of an RGB handle.
 * The rectangle is checked or computed when a sequence starts (again at every resolution change); the ratio limits 8:1 down and 1:4 up then apply
 * to crop -> rectangle.  A geometry that does not fit fails the handle, jm_amddec_last_error says why.  Stats: "rect_x", "rect_y", "rect_w", "rect_h"
 * (the rectangle in use: map model boxes back to the picture with it), "placed_frames", "sar_num", "sar_den" (as transmitted, 0 / 0 = absent).
 *   jm_amddec_fit_rect: the letterbox rectangle of a cw x ch picture with sample aspect ratio sar_num : sar_den (0 / 0: square) in a tw x th target,
 *     fit 1 or 2 (host only); rect = x, y, w, h.  Returns 0, -1 for invalid arguments.
 *   jm_amddec_scale_rect_device: jm_amddec_scale_device with a placement (rect_w / rect_h 0: to the target's edge; all 0: no placement) and a fill
 *     (-1 or 0xYYUUVV); same validation and return codes. */
int  jm_amddec_fit_rect(int cw, int ch, int sar_num, int sar_den, int tw, int th, int fit, int rect[4]);
int  jm_amddec_scale_rect_device(const void *d_src, int pitch, int chroma_offset, int w, int h, int lone_field, int crop_x, int crop_y, int crop_w,
                                 int crop_h, int tw, int th, int out_fmt, void *d_dst, void *stream, int rect_x, int rect_y, int rect_w, int rect_h,
                                 int fill);
/* Deinterlaced output (INTEGRATION.md "Deinterlaced output" defines the function D exactly).  With option "deinterlace" a handle hands out
 * C(R_G(D(F))): every display frame chosen by "deinterlace_when" keeps the lines of one field and rebuilds the others, before the resampler and
 * the colour conversion.  Options, before init (set_option returns -1 after init and for values out of range), all default 0:
 *   "deinterlace": 0 off, 1 bob (the missing lines are the rounded average of the kept lines above and below), 2 comb-adaptive (only where the
 *     woven frame is combed; static areas keep the full vertical resolution);
 *   "deinterlace_when": 0 auto -- the frames of an H.264 sequence with frame_mbs_only_flag = 0 (field pairs, frame pictures and lone fields;
 *     HEVC: never); 1 always -- every display frame of either codec;
 *   "deinterlace_field": 0 the field that is first in time (the smaller field order count; top on a tie or when there is one count only), 1 top,
 *     2 bottom.  A frame of which only one field was decoded is always interpolated from that field (bob), whatever the mode;
 *   "deinterlace_threshold": T of mode 2, 1..255 (0 = 10).
 *   "deinterlace_rate": 0 one frame per picture; 1 field rate -- every frame chosen for D leaves as TWO consecutive output frames, D with the
 *     field "deinterlace_field" picks kept, then D with the other field kept (a lone field: one frame).  No effect while "deinterlace" is 0.  Each
 *     decode / poll call still hands out one frame; the second of a pair is the next one.
 *   "deinterlace_temporal": 0 / 1 -- with "deinterlace" 2 a frame chosen for D is deinterlaced against the previous display frame (the function D3 of
 *     a missing sample is interpolated where one of the nine samples around it changed by more than T, and woven elsewhere) when
 *     that frame was chosen for D too, neither is a lone field and both belong to one activation; else as mode 2.  H.264 and HEVC; an MJPEG handle
 *     with the option set fails init.  Stats: "deint_temporal_frames", "display_temporal:<n>" (output frame n: 0 / 1).
 * Stats: "deint_frames" (output frames that went through D), "field_rate_pairs", "interlaced_sequence" (0 / 1, the active SPS), "display_field:<n>"
 * (output frame n: 0 not deinterlaced, 1 top kept, 2 bottom kept), "display_picture:<n>" (the display picture, index of "display_poc:<k>", that output
 * frame n shows), "out_fps_num" / "out_fps_den" (fps_num / fps_den, the numerator doubled while a field-rate handle deinterlaces the active sequence),
 * and with option "profile" k_deint_ns / _n / _pics / _alg_bytes (k_deint and k_deint2 together; a pair counts 2 frames and 3 / 2 of a frame's bytes).
 *   jm_amddec_deinterlace_device: stand-alone D on one pitch-linear NV12 surface in device memory (luma rows at `pitch`, the UV rows from byte
 *     chroma_offset; w x h even, h >= 4) into a pitch-linear NV12 surface (dst_pitch = w and dst_chroma_offset = w * h give a tight NV12 frame).
 *     mode 1 / 2, keep_field 1 top / 2 bottom, threshold 1..255 (0 = 10).  Source and destination must not overlap.  stream: a hipStream_t or
 *     NULL.  Returns 0, -1 for invalid arguments, or a negative hipError. */
int  jm_amddec_deinterlace_device(const void *d_src, int pitch, int chroma_offset, int w, int h, int mode, int keep_field, int threshold,
                                  void *d_dst, int dst_pitch, int dst_chroma_offset, void *stream);
/*   jm_amddec_deinterlace2_device: both fields of one surface in one pass (k_deint2) -- d_dst_first gets D with first_field (1 top / 2 bottom) kept,
 *     d_dst_second D with the other field kept, both in the destination layout above.  Arguments and returns as jm_amddec_deinterlace_device; in
 *     addition the two destinations must not overlap each other and neither may overlap the source (-1). */
int  jm_amddec_deinterlace2_device(const void *d_src, int pitch, int chroma_offset, int w, int h, int mode, int first_field, int threshold,
                                   void *d_dst_first, void *d_dst_second, int dst_pitch, int dst_chroma_offset, void *stream);
/*   jm_amddec_deinterlace3_device: the motion-adaptive deinterlacer D3 (option "deinterlace_temporal", k_deint3) -- d_src against d_prev, the surface
 *     of the previous display frame (same w x h, a pitch and chroma offset of its own): d_dst_first gets D3 with first_field (1 top / 2 bottom) kept
 *     and d_dst_second, unless NULL, D3 with the other field kept.  Arguments and returns as jm_amddec_deinterlace2_device (no mode: D3 is one
 *     function); -1 also for a NULL d_prev and for a destination that overlaps either source. */
int  jm_amddec_deinterlace3_device(const void *d_src, int pitch, int chroma_offset, const void *d_prev, int prev_pitch, int prev_chroma_offset, int w, int h,
                                   int first_field, int threshold, void *d_dst_first, void *d_dst_second, int dst_pitch, int dst_chroma_offset, void *stream);
/* RGB output (INTEGRATION.md "RGB output" defines the conversion C exactly).  A handle with an RGB spec hands out every display frame as
 * C(R_G(F)): three samples per pixel of the target size, planar (CHW) or interleaved (HWC), R,G,B or B,G,R order, u8 / f32 / f16 / bf16
 * (f16 and bf16 as their 16-bit patterns), frame bytes 3 * w * h * sizeof(sample).  matrix 0 / range 0 = from the stream's VUI (matrix: the VUI
 * value when supported, else BT.709 above 576 display lines and BT.601 otherwise; range: the VUI flag, else limited).  The float samples are
 * fl32(fl32(v * scale[c] / 16384) + bias[c]) of the 14-fractional-bit value v, per storage position c (scale / bias are ignored for u8).
 *   jm_amddec_set_rgb: before init; NULL = Y'CbCr output again.  0, or -1 after init or for an invalid spec.  output_frame, output_frame_device and
 *     feed_annexb then hand out RGB frames; output_argb_device and output_nv12_pitch_device return -1.  Stats: "out_frame_bytes" (of the frame
 *     current or about to be fetched), "rgb_frames", "color_matrix" / "color_range" (in use: H.273 MatrixCoefficients, 1 limited / 2 full),
 *     "vui_matrix" / "vui_primaries" / "vui_transfer" / "vui_full_range" (as transmitted, -1 = absent), "out_slot_bytes" (device + page-locked
 *     output-slot memory).  Without an explicit "job_slots" an RGB handle keeps at most 1 GiB of output slots (never fewer than 8 job slots).
 *   jm_amddec_color_coefs: the five 14-bit coefficients cy, crv, cgu, cgv, cbu of a matrix (1, 4, 5, 6, 7, 9) and range (host only); -1 unsupported.
 *   jm_amddec_rgb_device: stand-alone crop + resample + convert of one pitch-linear NV12 surface (arguments as jm_amddec_scale_device; matrix must
 *     be explicit, d_dst aligned to the sample size).  Returns 0, -1 for invalid arguments, or a negative hipError. */
typedef struct {
    int dtype;                  /* 0 u8, 1 f32, 2 f16, 3 bf16 */
    int planar;                 /* 1 CHW, 0 HWC */
    int bgr;                    /* 0 R,G,B; 1 B,G,R */
    int matrix;                 /* 0 auto (VUI), else 1, 4, 5, 6, 7, 9 */
    int range;                  /* 0 auto, 1 limited, 2 full */
    float scale[3], bias[3];    /* per storage position; ignored for u8 */
} jm_amddec_rgb_spec;
int  jm_amddec_set_rgb(jm_amddec_handle h, const jm_amddec_rgb_spec *spec);
int  jm_amddec_color_coefs(int matrix, int full_range, int coefs[5]);
int  jm_amddec_rgb_device(const void *d_src, int pitch, int chroma_offset, int w, int h, int lone_field, int crop_x, int crop_y, int crop_w,
                          int crop_h, int tw, int th, const jm_amddec_rgb_spec *spec, void *d_dst, void *stream);
/* ... with a placement and a fill (-1 or 0xRRGGBB), as jm_amddec_scale_rect_device: the fill goes through the sample step of the storage position
 * its colour lands in */
int  jm_amddec_rgb_rect_device(const void *d_src, int pitch, int chroma_offset, int w, int h, int lone_field, int crop_x, int crop_y, int crop_w,
                               int crop_h, int tw, int th, const jm_amddec_rgb_spec *spec, void *d_dst, void *stream, int rect_x, int rect_y,
                               int rect_w, int rect_h, int fill);
/* Interpolated chroma (INTEGRATION.md "RGB output" defines it exactly).  Options of an RGB handle, before init (set_option returns -1 after init and for
 * values out of range):
 *   "rgb_chroma": 0 (default) nearest chroma of the 4:2:0 frame at target size, as above; 1: the conversion is applied to a 4:4:4 frame whose chroma
 *     planes are the crop's chroma resampled straight to the full target at the stream's chroma sample location.  Without an RGB spec init fails and
 *     jm_amddec_last_error names the option.
 *   "chroma_loc": -1 (default) auto -- the VUI's chroma_sample_loc_type_top_field when present and 0..5, else 0; MJPEG: 1 --, 0..5: that location.  No
 *     effect without "rgb_chroma".  The frame's siting is applied to every frame handed out; per-field siting is not applied.
 * Stats: "vui_chroma_loc" / "vui_chroma_loc_bottom" (as transmitted, -1 = absent), "chroma_loc" (in use), "rgb_chroma", "rgb_chroma_frames", and with
 * option "profile" k_rgb_pack444_ns / _n / _pics (these frames count in k_rgb_pack_* and k_packout_* too).
 *   jm_amddec_chroma_taps: the tap table of one chroma axis, src_len chroma samples -> dst_len outputs of the full target with the siting shift q
 *     (-1, 0, +1 quarters of a chroma sample), in jm_amddec_scale_taps' layout and with its return values (host only); q = 0 is jm_amddec_scale_taps.
 *   jm_amddec_rgb_chroma_device: jm_amddec_rgb_rect_device with interpolated chroma at chroma_loc 0..5; same validation and return codes. */
int  jm_amddec_chroma_taps(int src_len, int dst_len, int q, int *first, short *weights, int max_taps);
int  jm_amddec_rgb_chroma_device(const void *d_src, int pitch, int chroma_offset, int w, int h, int lone_field, int crop_x, int crop_y, int crop_w,
                                 int crop_h, int tw, int th, const jm_amddec_rgb_spec *spec, void *d_dst, void *stream, int rect_x, int rect_y,
                                 int rect_w, int rect_h, int fill, int chroma_loc);
/* Picture hash verification (INTEGRATION.md "Picture hash" defines both hashes exactly).  An HEVC stream may say what every decoded picture hashes to:
 * the decoded picture hash SEI message (payload type 132) in a suffix SEI NAL unit (type 40) holds an MD5, a CRC or a checksum per colour component of
 * the picture at its coded size.  Option "verify_hash", before init (set_option returns -1 after init and for other values):
 *   0 (default) off: suffix SEI is not looked at and nothing changes;  1: the CRC or the checksum is computed on the device behind the picture's last
 *   kernel (k_hevc_pichash) and compared, mismatches are counted;  2: the first mismatch also fails the handle, jm_amddec_last_error then reads
 *   "picture hash mismatch: POC <n>, component <Y|Cb|Cr>, <crc|checksum> expected 0x... got 0x...".
 * Option "verify_md5", before init (0 default, 1; set_option returns -1 after init and for other values), takes effect only with verify_hash 1 or 2:
 *   0: MD5 messages (hash_type 0) are counted in "hash_md5" and never compared -- no kernel, table or allocation appears;  1: the three MD5 digests
 *   (RFC 1321, of each component's samples as a raster byte array of the coded size) are computed behind the picture's last kernel (k_hevc_md5) and
 *   compared; the picture counts in "hash_checked" like a CRC picture, and the error text reads "picture hash mismatch: POC <n>, component <Y|Cb|Cr>,
 *   md5 expected <32 hex digits> got <32 hex digits>".  An MD5 chain is serial: about 20 ms per 1080p picture, and the batch waits for it.
 * A hash in a prefix SEI is ignored; a malformed message counts in "errors" and is ignored.
 * Stats: "hash_pictures" (pictures that carried a hash message), "hash_checked", "hash_mismatch", "hash_unchecked" (their batch failed, or the handle
 * had), "hash_md5" (pictures that carried MD5), "hash_first_bad_poc" (-2^31: none), "hash_last_crc:<c>" / "hash_last_checksum:<c>" (c = 0..2: the device's values of the most
 * recently completed hashed picture), "hash_sei_poc:<n>" / "hash_sei_type:<n>" / "hash_sei_value:<n>:<c>" (the n-th hash message in decode order as
 * parsed; works on a parse_only handle), "hash_last_md5:<c>:<k>" (the device's digest of the most recent MD5-verified picture; k = 0..3: bytes
 * 4k .. 4k+3 of the 16 read big-endian, so four words printed %08x give the usual hex string), "hash_sei_md5:<n>:<c>:<k>" (the same view of the n-th
 * parsed message), and with option "profile" k_pichash_ns / _n / _pics / _alg_bytes and k_md5_ns / _n / _pics / _alg_bytes.
 *   jm_amddec_picture_hash_device: stand-alone, both hashes of one pitch-linear NV12 surface in device memory (luma rows at `pitch`, the UV rows from
 *     byte chroma_offset; w x h even, 2..16384): crc[c] and checksum[c] of Y, Cb, Cr.  stream: a hipStream_t or NULL; synchronised before returning.
 *     Returns 0, -1 for invalid arguments, or a negative hipError. */
int  jm_amddec_picture_hash_device(const void *d_src, int pitch, int chroma_offset, int w, int h, unsigned crc[3], unsigned checksum[3], void *stream);
/*   jm_amddec_picture_md5_device: its counterpart for MD5, same argument rules and return codes: md5[c] = the 16 digest bytes, RFC order, of Y, Cb, Cr. */
int  jm_amddec_picture_md5_device(const void *d_src, int pitch, int chroma_offset, int w, int h, unsigned char md5[3][16], void *stream);
/* SURVEY 8f f4 -- the encoder-side pre-processing of the reference (/root/reference/nv_enc/nv_enc.cpp:1022-1079: cuMemcpy2D of the luma plane +
 * the InterleaveUV kernel; the CPU loop of intel_enc.cpp:316-387) as one HIP kernel, device to device: a tight frame (src_fmt 1 = I420
 * planar Y,U,V; 0 = tight NV12) becomes a pitch-linear NV12 surface (luma rows at `pitch`, interleaved UV rows from row `height`), the layout an
 * encoder's input surface has.  width and height must be even, pitch >= width.
 *   jm_amddec_i420_to_nv12_device: stand-alone (any device frame).  stream: a hipStream_t or NULL.  Returns 0 or -1.
 *   jm_amddec_output_nv12_pitch_device: the same for the decoder's current display frame -- decode -> encoder surface without touching the host
 *     (the first half of the transcode loop the reference's README leaves unfinished).  Returns 0, or -1 when no frame is current. */
int  jm_amddec_i420_to_nv12_device(const void *d_src, int width, int height, int src_fmt, void *d_dst, int pitch, void *stream);
int  jm_amddec_output_nv12_pitch_device(void *dev_dst, int pitch, jm_amddec_handle h);

/* The hot loop of the reference harness in native code (/root/reference/test_nv_dec/test_nv_dec.cpp:184-250): feed the Annex-B buffer one
 * NAL unit per jm_nvdec_decode_frame call (a NAL = start code + payload up to the next start code, :63-86), fetch a frame with
 * jm_nvdec_output_frame into out_buf whenever got_frame == 1.  `passes` repeats the buffer.  Does not send end of stream (the caller
* decides when to drain).  out_buf == NULL (with option "device_output"): frames are taken with jm_amddec_output_frame_device instead, i.e. they
 * stay in device memory and nothing crosses PCIe (profiling: rocprofv3 replaces copy-engine transfers by blit kernels that disturb the decode
 * kernels).  Returns the number of frames fetched, < 0 on error.  Exists so that callers in interpreted languages
 * (bench.py) measure the library, not their own per-call overhead. */
long jm_amddec_feed_annexb(const unsigned char *buf, long len, int passes, unsigned char *out_buf, int out_cap, jm_amddec_handle handle);

#ifdef __cplusplus
}
#endif
#endif
