// jmcodec_amd/csrc/jm_amd_dec.cpp -- C ABI (include/jm_amd_dec.h) over jmamd::Decoder.
#include "../../include/jm_amd_dec.h"
#include "decoder.h"
#include "kernels.h"
#include "hevc_kernels.h"
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <vector>

using jmamd::Decoder;

// The engine drives several HIP streams (per lane: decode + pack-out, plus one copy stream) that must map to distinct
// hardware queues to run concurrently; ROCm's default is 4 queues per process.  Must be set before the runtime initialises.
__attribute__((constructor)) static void jm_amddec_runtime_defaults() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

// The host half is compiled for BMI1 / BMI2 / LZCNT (Makefile: the arithmetic decoder's variable shifts and leading-zero counts; every x86 host an
// MI355X is sold in has them).  A CPU without them gets told so before the first such instruction runs, instead of an illegal-instruction trap.
#if defined(__BMI2__) || defined(__BMI__) || defined(__LZCNT__)
__attribute__((constructor(101), target("no-bmi,no-bmi2,no-lzcnt"))) static void jm_amddec_cpu_check() {
    __builtin_cpu_init();
    if (!__builtin_cpu_supports("bmi") || !__builtin_cpu_supports("bmi2") || !__builtin_cpu_supports("lzcnt")) {
        fputs("jm_amd_dec: this build needs a CPU with BMI1, BMI2 and LZCNT (rebuild jmcodec_amd/csrc with HOST_ISA= for older hosts)\n", stderr);
        abort();
    }
}
#endif

#define D(h) (reinterpret_cast<Decoder *>(h))

// No C++ exception may cross the C ABI (a hostile stream must not be able to abort the host application through an allocation
// failure or a container bound): the entry points that run parser code convert them into the API's error return.
template <class F> static int guarded(jm_amddec_handle h, F &&f) {
    try { return f(); }
    catch (const std::exception &e) { D(h)->api_exception(e.what()); }
    catch (...) { D(h)->api_exception("unknown exception"); }
    return -1;
}

// The stand-alone *_device entry points run ONE job of an output kernel: upload it, launch(d_job, stream), wait for the stream, free it.
// 0, -1 (no memory for the job) or minus the HIP error the launch left
template <class Job, class Launch> static int run_one_job(const Job &job, void *stream, Launch &&launch) {
    Job *d_job = nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMalloc((void **)&d_job, sizeof job) != hipSuccess) return -1;
    hipMemcpyAsync(d_job, &job, sizeof job, hipMemcpyHostToDevice, st);
    launch(d_job, st);
    hipError_t e = hipGetLastError();
    hipStreamSynchronize(st);
    hipFree(d_job);
    return e == hipSuccess ? 0 : -(int)e;
}

// The placement arguments of the *_rect_device calls against the target: rect[] = x, y, w, h in use (w / h 0: to the target's edge); true: the picture
// is placed (the rectangle is not the whole target).  -1 in *bad: odd, negative or outside the target, or a fill outside -1 .. 0xFFFFFF
static bool resolve_rect(int tw, int th, int rx, int ry, int rw, int rh, long long fill, int rect[4], bool *bad) {
    *bad = true;
    if (((rx | ry | rw | rh) & 1) || rx < 0 || ry < 0 || rw < 0 || rh < 0 || fill < -1 || fill > 0xFFFFFF) return false;
    rect[0] = rx; rect[1] = ry; rect[2] = rw ? rw : tw - rx; rect[3] = rh ? rh : th - ry;
    if (rect[2] <= 0 || rect[3] <= 0 || rx + rect[2] > tw || ry + rect[3] > th) return false;
    *bad = false;
    return !(rx == 0 && ry == 0 && rect[2] == tw && rect[3] == th);
}

extern "C" {

__attribute__((visibility("default"))) jm_amddec_handle jm_amddec_create_handle(void) { return new Decoder(); }
__attribute__((visibility("default"))) int jm_amddec_init(int codec_type, int out_fmt, char *extra, int len, jm_amddec_handle h) {
    if (!h) return -1;
    return guarded(h, [&] { return D(h)->init(codec_type, out_fmt, reinterpret_cast<const uint8_t *>(extra), len); });
}
__attribute__((visibility("default"))) int jm_amddec_deinit(jm_amddec_handle h) { delete D(h); return 0; }
__attribute__((visibility("default"))) int jm_amddec_decode_frame(unsigned char *in_buf, int n, int *got, jm_amddec_handle h) {
    int dummy = 0;
    if (!h) return -1;
    return guarded(h, [&] { return D(h)->decode(in_buf, n, got ? got : &dummy); });
}
__attribute__((visibility("default"))) int jm_amddec_poll_frame(int *got, jm_amddec_handle h) {
    int dummy = 0;
    if (!h) return -1;
    return guarded(h, [&] { return D(h)->poll(got ? got : &dummy); });
}
__attribute__((visibility("default"))) int jm_amddec_wait_frame(int *got, int timeout_us, jm_amddec_handle h) {
    int dummy = 0;
    if (!h) return -1;
    return guarded(h, [&] { return D(h)->poll(got ? got : &dummy, timeout_us); });
}
__attribute__((visibility("default"))) int jm_amddec_push_data(unsigned char *in_buf, int n, jm_amddec_handle h) {
    if (!h) return -1;
    return guarded(h, [&] { return D(h)->push(in_buf, n); });
}
__attribute__((visibility("default"))) int jm_amddec_push_eos(jm_amddec_handle h) {
    if (!h) return -1;
    return guarded(h, [&] { return D(h)->push_eos(); });
}
__attribute__((visibility("default"))) int jm_amddec_output_frame(unsigned char *out, int *out_len, jm_amddec_handle h) {
    if (!h || !out || !out_len) return -1;
    return guarded(h, [&] { return D(h)->output(out, out_len); });
}
__attribute__((visibility("default"))) int jm_amddec_stream_info(int *w, int *hh, jm_amddec_handle h) { return D(h)->stream_info(w, hh); }
__attribute__((visibility("default"))) void jm_amddec_set_eof(int e, jm_amddec_handle h) { D(h)->set_eof(e != 0); }
__attribute__((visibility("default"))) int jm_amddec_is_exit(jm_amddec_handle h) { return D(h)->is_exit() ? 1 : 0; }
__attribute__((visibility("default"))) char *jm_amddec_show_dec_info(jm_amddec_handle h) { return D(h)->info(); }
__attribute__((visibility("default"))) int jm_amddec_is_hw_support(void) {      // nvdec_cuda_hw_support: device count > 0 (nv_dec.cpp:188-200)
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}
__attribute__((visibility("default"))) int jm_amddec_set_option(jm_amddec_handle h, const char *key, long long v) { return D(h)->set_option(key, v); }
__attribute__((visibility("default"))) long long jm_amddec_get_stat(jm_amddec_handle h, const char *key) { return D(h)->get_stat(key); }
__attribute__((visibility("default"))) const char *jm_amddec_last_error(jm_amddec_handle h) { return D(h)->last_error(); }
__attribute__((visibility("default"))) int jm_amddec_output_frame_device(void **dev, int *len, jm_amddec_handle h) {
    return (h && dev && len) ? D(h)->output_device(dev, len) : -1; }
__attribute__((visibility("default"))) int jm_amddec_output_argb_device(void *dev_dst, int pitch, jm_amddec_handle h) {
    return (h && dev_dst) ? D(h)->output_argb_device(dev_dst, pitch) : -1; }
__attribute__((visibility("default"))) int jm_amddec_output_nv12_pitch_device(void *dev_dst, int pitch, jm_amddec_handle h) {
    return (h && dev_dst) ? D(h)->output_nv12_pitch_device(dev_dst, pitch) : -1; }
__attribute__((visibility("default"))) int jm_amddec_i420_to_nv12_device(const void *d_src, int width, int height, int src_fmt, void *d_dst, int pitch,
    void *stream) {
    if (!d_src || !d_dst || width <= 0 || height <= 0 || (width & 1) || (height & 1) || pitch < width || (src_fmt != 0 && src_fmt != 1)) return -1;
    jmamd::launch_frame_to_nv12_pitch((const uint8_t *)d_src, width, height, src_fmt, (uint8_t *)d_dst, pitch, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
__attribute__((visibility("default"))) int jm_amddec_packout_device(const void *src, int pitch, int w, int hgt, int fmt, void *dst, void *stream) {
    jmamd::PackJob job{static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst), pitch, pitch * hgt, w, hgt, fmt, 0};
    return run_one_job(job, stream, [&](const jmamd::PackJob *d_job, hipStream_t st) { jmamd::launch_packout(d_job, 1, w, hgt, st); });
}

__attribute__((visibility("default"))) int jm_amddec_scale_taps(int src_len, int dst_len, int *first, short *weights, int max_taps) {
    std::vector<int32_t> f; std::vector<int16_t> w;
    const int taps = jmamd::build_scale_taps(src_len, dst_len, f, w);
    if (taps < 0 || !first || !weights) return taps;          // (no buffers: how many taps a table of this ratio has)
    if (taps > max_taps) return -1;
    for (int j = 0; j < dst_len; j++) {
        first[j] = f[j];
        for (int k = 0; k < max_taps; k++) weights[(size_t)j * max_taps + k] = k < taps ? w[(size_t)j * taps + k] : 0;
    }
    return taps;
}
// ... and of a chroma plane to the full target with the siting shift q (INTEGRATION.md "RGB output": interpolated chroma)
__attribute__((visibility("default"))) int jm_amddec_chroma_taps(int src_len, int dst_len, int q, int *first, short *weights, int max_taps) {
    std::vector<int32_t> f; std::vector<int16_t> w;
    const int taps = jmamd::build_chroma_taps(src_len, dst_len, q, f, w);
    if (taps < 0 || !first || !weights) return taps;
    if (taps > max_taps) return -1;
    for (int j = 0; j < dst_len; j++) {
        first[j] = f[j];
        for (int k = 0; k < max_taps; k++) weights[(size_t)j * max_taps + k] = k < taps ? w[(size_t)j * taps + k] : 0;
    }
    return taps;
}
__attribute__((visibility("default"))) int jm_amddec_fit_rect(int cw, int ch, int sar_num, int sar_den, int tw, int th, int fit, int rect[4]) {
    return jmamd::fit_rect(cw, ch, sar_num, sar_den, tw, th, fit, rect) ? 0 : -1;
}
__attribute__((visibility("default"))) int jm_amddec_scale_device(const void *src, int pitch, int chroma_offset, int w, int hgt, int lone_field, int crop_x,
    int crop_y, int crop_w, int crop_h, int tw, int th, int out_fmt, void *dst, void *stream) {
    return jm_amddec_scale_rect_device(src, pitch, chroma_offset, w, hgt, lone_field, crop_x, crop_y, crop_w, crop_h, tw, th, out_fmt, dst, stream, 0, 0, 0, 0, -1);
}
// ... with the picture placed in the target (INTEGRATION.md "Placed output"); the ratio limits apply to the rectangle
__attribute__((visibility("default"))) int jm_amddec_scale_rect_device(const void *src, int pitch, int chroma_offset, int w, int hgt, int lone_field, int crop_x,
    int crop_y, int crop_w, int crop_h, int tw, int th, int out_fmt, void *dst, void *stream, int rect_x, int rect_y, int rect_w, int rect_h, int fill) {
    if (!src || !dst || w <= 0 || hgt <= 0 || pitch < w || lone_field < 0 || lone_field > 2 || (out_fmt != 0 && out_fmt != 1)) return -1;
    if ((crop_x | crop_y | crop_w | crop_h | tw | th) & 1) return -1;
    if (crop_x < 0 || crop_y < 0 || crop_w <= 0 || crop_h <= 0 || crop_x + crop_w > w || crop_y + crop_h > hgt || tw <= 0 || th <= 0) return -1;
    int rc[4]; bool bad;
    const bool placed = resolve_rect(tw, th, rect_x, rect_y, rect_w, rect_h, fill, rc, &bad);
    if (bad) return -1;
    if (crop_w > 8 * rc[2] || crop_h > 8 * rc[3] || rc[2] > 4 * crop_w || rc[3] > 4 * crop_h) return -1;
    jmamd::ScaleJob job{static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst), pitch, chroma_offset, crop_x, crop_y, tw, th, out_fmt, lone_field, {}};
    if (placed) { job.rx = rc[0]; job.ry = rc[1]; job.rw = rc[2]; job.rh = rc[3]; job.fill = fill < 0 ? 0x108080 : (int)fill; }
    uint8_t *tables = nullptr;
    if (!jmamd::upload_scale_tables(crop_w, crop_h, rc[2], rc[3], &tables, job.ax)) return -1;
    const int r = run_one_job(job, stream, [&](const jmamd::ScaleJob *d_job, hipStream_t st) {
        jmamd::launch_scale_pack(d_job, 1, jmamd::scale_tiles(tw, th), st); });
    hipFree(tables);
    return r;
}

__attribute__((visibility("default"))) int jm_amddec_deinterlace_device(const void *src, int pitch, int chroma_offset, int w, int hgt, int mode, int keep_field,
    int threshold, void *dst, int dst_pitch, int dst_chroma_offset, void *stream) {
    if (!src || !dst || w <= 0 || hgt < 4 || ((w | hgt) & 1) || pitch < w || dst_pitch < w) return -1;
    if ((mode != 1 && mode != 2) || (keep_field != 1 && keep_field != 2) || threshold < 0 || threshold > 255) return -1;
    if (chroma_offset < 0 || dst_chroma_offset < 0) return -1;
    const int t = threshold ? threshold : 10;
    jmamd::DeintJob job{static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst), pitch, chroma_offset, w, hgt, dst_pitch, dst_chroma_offset, 0, mode,
        keep_field - 1, 4 * t * t};
    return run_one_job(job, stream, [&](const jmamd::DeintJob *d_job, hipStream_t st) { jmamd::launch_deint(d_job, 1, jmamd::deint_items(w, hgt), st); });
}

// both fields of one surface in one pass (k_deint2): D with first_field kept, then D with the other field kept
__attribute__((visibility("default"))) int jm_amddec_deinterlace2_device(const void *src, int pitch, int chroma_offset, int w, int hgt, int mode, int first_field,
    int threshold, void *dst_first, void *dst_second, int dst_pitch, int dst_chroma_offset, void *stream) {
    if (!src || !dst_first || !dst_second || w <= 0 || hgt < 4 || ((w | hgt) & 1) || pitch < w || dst_pitch < w) return -1;
    if ((mode != 1 && mode != 2) || (first_field != 1 && first_field != 2) || threshold < 0 || threshold > 255) return -1;
    if (chroma_offset < 0 || dst_chroma_offset < 0) return -1;
    {   // the two destinations must not overlap each other, and neither may overlap the source (every row is read after rows of both were written)
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)chroma_offset + (size_t)pitch * (hgt / 2 - 1) + w;
        const size_t dn = (size_t)dst_chroma_offset + (size_t)dst_pitch * (hgt / 2 - 1) + w;
        const uintptr_t a0 = (uintptr_t)dst_first, a1 = a0 + dn, b0 = (uintptr_t)dst_second, b1 = b0 + dn;
        if ((a0 < b1 && b0 < a1) || (a0 < s1 && s0 < a1) || (b0 < s1 && s0 < b1)) return -1;
    }
    const int t = threshold ? threshold : 10;
    jmamd::DeintJob job{static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst_first), pitch, chroma_offset, w, hgt, dst_pitch, dst_chroma_offset, 0, mode,
        first_field - 1, 4 * t * t, static_cast<uint8_t *>(dst_second)};
    return run_one_job(job, stream, [&](const jmamd::DeintJob *d_job, hipStream_t st) { jmamd::launch_deint2(d_job, 1, jmamd::deint2_items(w, hgt), st); });
}

// the motion-adaptive deinterlacer D3 on one surface and the surface of the previous frame (k_deint3): first_field kept, and -- when d_dst_second is
// given -- the other field kept as well
__attribute__((visibility("default"))) int jm_amddec_deinterlace3_device(const void *src, int pitch, int chroma_offset, const void *prev, int prev_pitch,
    int prev_chroma_offset, int w, int hgt, int first_field, int threshold, void *dst_first, void *dst_second, int dst_pitch, int dst_chroma_offset, void *stream) {
    if (!src || !prev || !dst_first || w <= 0 || hgt < 4 || ((w | hgt) & 1) || pitch < w || prev_pitch < w || dst_pitch < w) return -1;
    if ((first_field != 1 && first_field != 2) || threshold < 0 || threshold > 255) return -1;
    if (chroma_offset < 0 || prev_chroma_offset < 0 || dst_chroma_offset < 0) return -1;
    {   // no destination may overlap either source, nor the other destination
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)chroma_offset + (size_t)pitch * (hgt / 2 - 1) + w;
        const uintptr_t q0 = (uintptr_t)prev, q1 = q0 + (size_t)prev_chroma_offset + (size_t)prev_pitch * (hgt / 2 - 1) + w;
        const size_t dn = (size_t)dst_chroma_offset + (size_t)dst_pitch * (hgt / 2 - 1) + w;
        const uintptr_t a0 = (uintptr_t)dst_first, a1 = a0 + dn, b0 = (uintptr_t)dst_second, b1 = b0 + dn;
        if ((a0 < s1 && s0 < a1) || (a0 < q1 && q0 < a1)) return -1;
        if (dst_second && ((a0 < b1 && b0 < a1) || (b0 < s1 && s0 < b1) || (b0 < q1 && q0 < b1))) return -1;
    }
    const int t = threshold ? threshold : 10;
    jmamd::DeintJob job{static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst_first), pitch, chroma_offset, w, hgt, dst_pitch, dst_chroma_offset, 0, 2,
        first_field - 1, 4 * t * t, static_cast<uint8_t *>(dst_second), static_cast<const uint8_t *>(prev), prev_pitch, prev_chroma_offset, t};
    return run_one_job(job, stream, [&](const jmamd::DeintJob *d_job, hipStream_t st) { jmamd::launch_deint3(d_job, 1, jmamd::deint2_items(w, hgt), st); });
}

// the two parallel picture hashes of one surface: the kernel the decoder runs behind a picture with a hash SEI, on a one-picture batch
__attribute__((visibility("default"))) int jm_amddec_picture_hash_device(const void *src, int pitch, int chroma_offset, int w, int hgt, unsigned crc[3],
    unsigned checksum[3], void *stream) {
    if (!src || !crc || !checksum || w < 2 || hgt < 2 || ((w | hgt) & 1) || w > 16384 || hgt > 16384 || pitch < w || chroma_offset < 0) return -1;
    jmamd::HevcPicParams pp = {};
    pp.w = w; pp.h = hgt; pp.pitch = pitch; pp.chroma_offset = chroma_offset; pp.cur = 0; pp.hash_mode = 1;
    pp.surf[0] = static_cast<uint8_t *>(const_cast<void *>(src));
    uint32_t *d_hash = nullptr, words[6] = {0, 0, 0, 0, 0, 0};
    if (hipMalloc((void **)&d_hash, sizeof(uint32_t) * jmamd::kHashStride) != hipSuccess) return -1;
    int r = run_one_job(pp, stream, [&](const jmamd::HevcPicParams *d_pp, hipStream_t st) {
        jmamd::launch_hevc_pichash(d_pp, 1, hgt, d_hash, st);
        hipMemcpyAsync(words, d_hash, sizeof words, hipMemcpyDeviceToHost, st); });
    hipFree(d_hash);
    if (r == 0) for (int c = 0; c < 3; c++) { crc[c] = words[c]; checksum[c] = words[3 + c]; }
    return r;
}

// ... and its three MD5s: k_hevc_md5 on a one-picture batch
__attribute__((visibility("default"))) int jm_amddec_picture_md5_device(const void *src, int pitch, int chroma_offset, int w, int hgt, unsigned char md5[3][16],
    void *stream) {
    if (!src || !md5 || w < 2 || hgt < 2 || ((w | hgt) & 1) || w > 16384 || hgt > 16384 || pitch < w || chroma_offset < 0) return -1;
    jmamd::HevcPicParams pp = {};
    pp.w = w; pp.h = hgt; pp.pitch = pitch; pp.chroma_offset = chroma_offset; pp.cur = 0; pp.hash_mode = 2;
    pp.surf[0] = static_cast<uint8_t *>(const_cast<void *>(src));
    uint32_t *d_hash = nullptr, words[12] = {};
    if (hipMalloc((void **)&d_hash, sizeof(uint32_t) * jmamd::kHashStride) != hipSuccess) return -1;
    int r = run_one_job(pp, stream, [&](const jmamd::HevcPicParams *d_pp, hipStream_t st) {
        jmamd::launch_hevc_md5(d_pp, 1, d_hash, st);
        hipMemcpyAsync(words, d_hash + jmamd::kMd5Word, sizeof words, hipMemcpyDeviceToHost, st); });
    hipFree(d_hash);
    if (r == 0) memcpy(md5, words, 48);
    return r;
}

static_assert(sizeof(jm_amddec_rgb_spec) == sizeof(jmamd::RgbSpec) && offsetof(jm_amddec_rgb_spec, bias) == offsetof(jmamd::RgbSpec, bias),
              "RgbSpec restates jm_amddec_rgb_spec");
__attribute__((visibility("default"))) int jm_amddec_set_rgb(jm_amddec_handle h, const jm_amddec_rgb_spec *spec) {
    if (!h) return -1;
    return D(h)->set_rgb(reinterpret_cast<const jmamd::RgbSpec *>(spec));
}
__attribute__((visibility("default"))) int jm_amddec_color_coefs(int matrix, int full_range, int coefs[5]) {
    int c[5];
    if (!jmamd::color_coefs(matrix, full_range != 0, c)) return -1;
    if (coefs) for (int k = 0; k < 5; k++) coefs[k] = c[k];
    return 0;
}
__attribute__((visibility("default"))) int jm_amddec_rgb_device(const void *src, int pitch, int chroma_offset, int w, int hgt, int lone_field, int crop_x,
    int crop_y, int crop_w, int crop_h, int tw, int th, const jm_amddec_rgb_spec *spec, void *dst, void *stream) {
    return jm_amddec_rgb_rect_device(src, pitch, chroma_offset, w, hgt, lone_field, crop_x, crop_y, crop_w, crop_h, tw, th, spec, dst, stream, 0, 0, 0, 0, -1);
}
// ... with the picture placed in the target; a placed job whose rectangle has the crop's size (pure padding) reads the surface directly
static int rgb_rect_device(const void *src, int pitch, int chroma_offset, int w, int hgt, int lone_field, int crop_x, int crop_y, int crop_w, int crop_h, int tw,
    int th, const jm_amddec_rgb_spec *spec, void *dst, void *stream, int rect_x, int rect_y, int rect_w, int rect_h, int fill, int chroma_loc);
__attribute__((visibility("default"))) int jm_amddec_rgb_rect_device(const void *src, int pitch, int chroma_offset, int w, int hgt, int lone_field, int crop_x,
    int crop_y, int crop_w, int crop_h, int tw, int th, const jm_amddec_rgb_spec *spec, void *dst, void *stream, int rect_x, int rect_y, int rect_w, int rect_h,
    int fill) {
    return rgb_rect_device(src, pitch, chroma_offset, w, hgt, lone_field, crop_x, crop_y, crop_w, crop_h, tw, th, spec, dst, stream, rect_x, rect_y, rect_w, rect_h, fill, -1);
}
// ... with interpolated chroma at chroma_sample_loc_type chroma_loc (k_rgb_pack444): every geometry goes through the tap tables
__attribute__((visibility("default"))) int jm_amddec_rgb_chroma_device(const void *src, int pitch, int chroma_offset, int w, int hgt, int lone_field, int crop_x,
    int crop_y, int crop_w, int crop_h, int tw, int th, const jm_amddec_rgb_spec *spec, void *dst, void *stream, int rect_x, int rect_y, int rect_w, int rect_h,
    int fill, int chroma_loc) {
    if (chroma_loc < 0 || chroma_loc > 5) return -1;
    return rgb_rect_device(src, pitch, chroma_offset, w, hgt, lone_field, crop_x, crop_y, crop_w, crop_h, tw, th, spec, dst, stream, rect_x, rect_y, rect_w, rect_h, fill, chroma_loc);
}
// (chroma_loc -1: nearest chroma, k_rgb_pack)
static int rgb_rect_device(const void *src, int pitch, int chroma_offset, int w, int hgt, int lone_field, int crop_x, int crop_y, int crop_w, int crop_h, int tw,
    int th, const jm_amddec_rgb_spec *spec, void *dst, void *stream, int rect_x, int rect_y, int rect_w, int rect_h, int fill, int chroma_loc) {
    if (!src || !dst || !spec || w <= 0 || hgt <= 0 || pitch < w || lone_field < 0 || lone_field > 2) return -1;
    const jmamd::RgbSpec &s = *reinterpret_cast<const jmamd::RgbSpec *>(spec);
    if (!jmamd::rgb_spec_valid(s, true) || ((uintptr_t)dst % (uintptr_t)jmamd::rgb_sample_bytes(s.dtype))) return -1;
    if ((crop_x | crop_y | crop_w | crop_h | tw | th) & 1) return -1;
    if (crop_x < 0 || crop_y < 0 || crop_w <= 0 || crop_h <= 0 || crop_x + crop_w > w || crop_y + crop_h > hgt || tw <= 0 || th <= 0) return -1;
    int rc[4]; bool bad;
    const bool placed = resolve_rect(tw, th, rect_x, rect_y, rect_w, rect_h, fill, rc, &bad);
    if (bad) return -1;
    if (crop_w > 8 * rc[2] || crop_h > 8 * rc[3] || rc[2] > 4 * crop_w || rc[3] > 4 * crop_h) return -1;
    jmamd::RgbJob job = {};
    job.s = jmamd::ScaleJob{static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst), pitch, chroma_offset, crop_x, crop_y, tw, th, 0, lone_field, {}};
    if (placed) { job.s.rx = rc[0]; job.s.ry = rc[1]; job.s.rw = rc[2]; job.s.rh = rc[3]; job.fill = fill < 0 ? 0 : (int)fill; }
    job.identity = chroma_loc < 0 && rc[2] == crop_w && rc[3] == crop_h;
    job.chroma = chroma_loc >= 0;
    jmamd::fill_rgb_color(job, s, s.matrix, s.range == 2);
    uint8_t *tables = nullptr, *ctables = nullptr;
    if (!job.identity && !jmamd::upload_scale_tables(crop_w, crop_h, rc[2], rc[3], &tables, job.s.ax)) return -1;
    if (job.chroma && !jmamd::upload_chroma_tables(crop_w, crop_h, rc[2], rc[3], chroma_loc, &ctables, job.cax)) { hipFree(tables); return -1; }
    const int tiles = jmamd::rgb_tiles(tw, th);
    const int r = run_one_job(job, stream, [&](const jmamd::RgbJob *d_job, hipStream_t st) {
        jmamd::launch_rgb_pack(d_job, 1, !job.chroma && job.identity ? tiles : 0, !job.chroma && !job.identity ? tiles : 0, job.chroma ? tiles : 0, st); });
    if (tables) hipFree(tables);
    if (ctables) hipFree(ctables);
    return r;
}

__attribute__((visibility("default"))) long jm_amddec_feed_annexb(const unsigned char *buf, long len, int passes, unsigned char *out, int out_cap,
    jm_amddec_handle h) {
    // VP8 has no start codes to cut at: the call is refused for codec_type 5 (feed an IVF stream or one frame per call through jm_amddec_decode_frame)
    if (h && D(h)->codec() == 5) { D(h)->refuse_call("jm_amddec_feed_annexb is not available for VP8 (codec_type 5): the stream has no start codes"); return -1; }
    if (!h || !buf || len < 4) return -1;       // out == NULL: frames stay on the device (jm_amddec_output_frame_device), nothing is copied
    // NAL boundaries as find_nalu sees them: a start code is 00 00 01, or 00 00 00 01 (then the NAL starts one byte earlier)
    std::vector<long> starts;
    for (long i = 0; i + 3 <= len; i++) if (buf[i] == 0 && buf[i + 1] == 0 && buf[i + 2] == 1) { long s0 = (i > 0 && buf[i - 1] == 0) ? i - 1 : i;
        if (starts.empty() || s0 > starts.back()) starts.push_back(s0); i += 2; }
    if (starts.empty()) return -1;
    long frames = 0;
    for (int p = 0; p < passes; p++)
        for (size_t k = 0; k < starts.size(); k++) {
            const long b = starts[k], e = k + 1 < starts.size() ? starts[k + 1] : len;
            int got = 0;
            if (guarded(h, [&] { return D(h)->decode(buf + b, (int)(e - b), &got); }) != 0) return -2;
            // (a field-rate handle puts out up to two frames per picture: one more look, so that finished frames do not pile up behind the input)
            for (int take = 0; got == 1 && take < (D(h)->field_rate() ? 2 : 1); take++) {
                if (out) { int n = out_cap; if (D(h)->output(out, &n) > 0) frames++; }
                else { void *dev = nullptr; int n = 0; if (D(h)->output_device(&dev, &n) > 0) frames++; }
                if (take == 0 && D(h)->field_rate() && guarded(h, [&] { return D(h)->poll(&got); }) != 0) return -2;
            }
        }
    return frames;
}

}  // extern "C"
