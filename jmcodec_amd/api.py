"""ctypes binding of ``include/jm_amd_dec.h`` plus a Python mirror of the reference API.

Mirrors /root/reference/nv_dec/jm_nv_dec.h:27-88 (``jm_nvdec_*``) and the call loop of
/root/reference/test_nv_dec/test_nv_dec.cpp:163-259.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = None


def lib_path():
    # JM_AMD_DEC_LIB: developer aid (timing experiments with alternative builds of the library); the product is lib/libjm_amd_dec.so
    return os.environ.get("JM_AMD_DEC_LIB") or os.path.join(_HERE, "lib", "libjm_amd_dec.so")


def build(force=False):
    """Compile the HIP/C++ sources in-tree (hipcc --offload-arch=gfx950)."""
    if force or not os.path.exists(lib_path()) or _stale():
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return lib_path()


def _stale():
    try:
        t = os.path.getmtime(lib_path())
        src = os.path.join(_HERE, "csrc")
        return any(os.path.getmtime(os.path.join(src, f)) > t for f in os.listdir(src))
    except OSError:
        return True


def lib():
    """Load libjm_amd_dec.so; raises (never falls back) when it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run jmcodec_amd.build() / __graft_entry__.build() first "
                           "(the HIP backend is mandatory, there is no CPU fallback)")
    L = C.CDLL(path)
    vp, cp, ip = C.c_void_p, C.c_char_p, C.POINTER(C.c_int)
    L.jm_amddec_create_handle.restype = vp
    L.jm_amddec_init.argtypes = [C.c_int, C.c_int, cp, C.c_int, vp]
    L.jm_amddec_deinit.argtypes = [vp]
    L.jm_amddec_decode_frame.argtypes = [vp, C.c_int, ip, vp]
    L.jm_amddec_output_frame.argtypes = [vp, ip, vp]
    L.jm_amddec_stream_info.argtypes = [ip, ip, vp]
    L.jm_amddec_set_eof.argtypes = [C.c_int, vp]
    L.jm_amddec_set_eof.restype = None
    L.jm_amddec_is_exit.argtypes = [vp]
    L.jm_amddec_show_dec_info.argtypes = [vp]
    L.jm_amddec_show_dec_info.restype = cp
    L.jm_amddec_set_option.argtypes = [vp, cp, C.c_longlong]
    L.jm_amddec_get_stat.argtypes = [vp, cp]
    L.jm_amddec_get_stat.restype = C.c_longlong
    L.jm_amddec_last_error.argtypes = [vp]
    L.jm_amddec_last_error.restype = cp
    L.jm_amddec_packout_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.jm_amddec_output_frame_device.argtypes = [C.POINTER(C.c_void_p), ip, vp]
    L.jm_amddec_scale_taps.argtypes = [C.c_int, C.c_int, ip, C.POINTER(C.c_short), C.c_int]
    L.jm_amddec_scale_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, vp, vp]
    L.jm_amddec_scale_rect_device.argtypes = L.jm_amddec_scale_device.argtypes + [C.c_int] * 5
    L.jm_amddec_fit_rect.argtypes = [C.c_int] * 7 + [ip]
    L.jm_amddec_deinterlace_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]
    L.jm_amddec_deinterlace2_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp]
    if hasattr(L, "jm_amddec_deinterlace3_device"):      # (a library of before the call, loaded through JM_AMD_DEC_LIB by the bench tools, lacks it)
        L.jm_amddec_deinterlace3_device.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp]
    L.jm_amddec_feed_annexb.argtypes = [cp, C.c_long, C.c_int, C.POINTER(C.c_ubyte), C.c_int, vp]
    L.jm_amddec_feed_annexb.restype = C.c_long
    L.jm_amddec_poll_frame.argtypes = [ip, vp]
    L.jm_amddec_wait_frame.argtypes = [ip, C.c_int, vp]
    L.jm_amddec_push_data.argtypes = [vp, C.c_int, vp]
    # push / pull API (include/jm_amd_intel_dec.h <- /root/reference/intel_dec/jm_intel_dec.h:29-122)
    L.jm_amdintel_create_handle.restype = vp
    L.jm_amdintel_init.argtypes = [C.c_int, C.c_int, vp]
    L.jm_amdintel_deinit.argtypes = [vp]
    L.jm_amdintel_set_yuv_callback.argtypes = [vp, vp, vp]
    L.jm_amdintel_input_data.argtypes = [vp, C.c_int, vp]
    L.jm_amdintel_output_frame.argtypes = [vp, ip, vp]
    L.jm_amdintel_set_eof.argtypes = [C.c_int, vp]
    L.jm_amdintel_info.argtypes = [vp]
    L.jm_amdintel_info.restype = cp
    L.jm_amdintel_get_stream_info.argtypes = [ip, ip, C.POINTER(C.c_float), vp]
    L.jm_amdintel_need_more_data.argtypes = [vp]
    L.jm_amdintel_free_buf_len.argtypes = [vp]
    L.jm_amdintel_is_exit.argtypes = [vp]
    L.jm_amdintel_run_pushpull.argtypes = [cp, C.c_long, C.POINTER(C.c_ubyte), C.c_int, vp]
    L.jm_amdintel_run_pushpull.restype = C.c_long
    L.jm_amdintel_decoder.argtypes = [vp]
    L.jm_amdintel_decoder.restype = vp
    L.jm_amddec_set_rgb.argtypes = [vp, C.POINTER(RgbSpec)]
    L.jm_amddec_color_coefs.argtypes = [C.c_int, C.c_int, ip]
    L.jm_amddec_rgb_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(RgbSpec), vp, vp]
    L.jm_amddec_rgb_rect_device.argtypes = L.jm_amddec_rgb_device.argtypes + [C.c_int] * 5
    L.jm_amddec_rgb_chroma_device.argtypes = L.jm_amddec_rgb_rect_device.argtypes + [C.c_int]
    L.jm_amddec_chroma_taps.argtypes = [C.c_int, C.c_int, C.c_int, ip, C.POINTER(C.c_short), C.c_int]
    L.jm_amddec_picture_hash_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint), vp]
    L.jm_amddec_picture_md5_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte * 16), vp]
    _LIB = L
    return L


# ---- the reference's ten functions, same names and argument order -------------------------
def jm_nvdec_is_hw_support():
    return bool(lib().jm_amddec_is_hw_support())


def jm_nvdec_create_handle():
    return lib().jm_amddec_create_handle()


def jm_nvdec_init(codec_type, out_fmt, extra_data, length, handle):
    return lib().jm_amddec_init(codec_type, out_fmt, extra_data, length, handle)


def jm_nvdec_deinit(handle):
    return lib().jm_amddec_deinit(handle)


def jm_nvdec_decode_frame(in_buf, in_data_len, handle):
    """Returns (ret, got_frame).  in_buf: bytes / ctypes buffer / None."""
    got = C.c_int(0)
    if in_buf is None or in_data_len == 0:
        ret = lib().jm_amddec_decode_frame(None, 0, C.byref(got), handle)
    else:
        if isinstance(in_buf, (bytes, bytearray)):
            in_buf = C.cast(C.c_char_p(bytes(in_buf)), C.c_void_p)
        ret = lib().jm_amddec_decode_frame(in_buf, in_data_len, C.byref(got), handle)
    return ret, got.value


def jm_nvdec_output_frame(out_buf, out_len, handle):
    """out_buf: writable ctypes buffer; out_len: its capacity.  Returns (ret, bytes_written)."""
    n = C.c_int(out_len)
    ret = lib().jm_amddec_output_frame(C.cast(out_buf, C.c_void_p), C.byref(n), handle)
    return ret, n.value


def jm_nvdec_stream_info(handle):
    w, h = C.c_int(0), C.c_int(0)
    lib().jm_amddec_stream_info(C.byref(w), C.byref(h), handle)
    return w.value, h.value


def jm_nvdec_set_eof(is_eof, handle):
    lib().jm_amddec_set_eof(1 if is_eof else 0, handle)


def jm_nvdec_is_exit(handle):
    return bool(lib().jm_amddec_is_exit(handle))


def jm_nvdec_show_dec_info(handle):
    return lib().jm_amddec_show_dec_info(handle).decode()


# ---- scaled and cropped output (include/jm_amd_dec.h; the resampler is defined in INTEGRATION.md) ----------
def scale_taps(src_len, dst_len, max_taps=9):
    """Tap table of one axis, src_len -> dst_len samples: (first, weights) -- first[j] the first source sample of output j (not clamped),
    weights[j] the list of its weights (1/16384) for source samples clamp(first[j] + k).  None when the ratio is invalid."""
    first, w = (C.c_int * max(dst_len, 1))(), (C.c_short * max(dst_len * max_taps, 1))()
    taps = lib().jm_amddec_scale_taps(src_len, dst_len, first, w, max_taps)
    if taps < 0:
        return None
    return list(first[:dst_len]), [list(w[j * max_taps:j * max_taps + taps]) for j in range(dst_len)]


def deinterlace_device(src, pitch, chroma_offset, width, height, mode, keep_field, dst, dst_pitch=None, dst_chroma_offset=None, threshold=0, stream=None):
    """jm_amddec_deinterlace_device: the deinterlacer D (INTEGRATION.md "Deinterlaced output") on one pitch-linear NV12 surface; mode 1 bob / 2
    comb-adaptive, keep_field 1 top / 2 bottom; src / dst device addresses (dst: a tight NV12 frame unless a pitch and a chroma offset are given).
    Returns 0 or < 0."""
    dp = width if dst_pitch is None else dst_pitch
    return lib().jm_amddec_deinterlace_device(src, pitch, chroma_offset, width, height, mode, keep_field, threshold, dst, dp,
                                              dp * height if dst_chroma_offset is None else dst_chroma_offset, stream)


def deinterlace2_device(src, pitch, chroma_offset, width, height, mode, first_field, dst_first, dst_second, dst_pitch=None, dst_chroma_offset=None,
                        threshold=0, stream=None):
    """jm_amddec_deinterlace2_device: field-rate deinterlacing of one pitch-linear NV12 surface in one pass -- dst_first gets D with first_field
    (1 top / 2 bottom) kept, dst_second D with the other field kept; both in deinterlace_device's destination layout.  The destinations must not
    overlap each other or the source.  Returns 0 or < 0."""
    dp = width if dst_pitch is None else dst_pitch
    return lib().jm_amddec_deinterlace2_device(src, pitch, chroma_offset, width, height, mode, first_field, threshold, dst_first, dst_second, dp,
                                               dp * height if dst_chroma_offset is None else dst_chroma_offset, stream)


def deinterlace3_device(src, pitch, chroma_offset, prev, prev_pitch, prev_chroma_offset, width, height, first_field, dst_first, dst_second=None,
                        dst_pitch=None, dst_chroma_offset=None, threshold=0, stream=None):
    """jm_amddec_deinterlace3_device: the motion-adaptive deinterlacer D3 (INTEGRATION.md "Deinterlaced output") on one pitch-linear NV12 surface
    against the surface of the previous display frame -- dst_first gets D3 with first_field (1 top / 2 bottom) kept, dst_second (optional) D3 with
    the other field kept; both in deinterlace_device's destination layout.  No destination may overlap a source or the other destination.
    Returns 0 or < 0."""
    dp = width if dst_pitch is None else dst_pitch
    return lib().jm_amddec_deinterlace3_device(src, pitch, chroma_offset, prev, prev_pitch, prev_chroma_offset, width, height, first_field, threshold,
                                               dst_first, dst_second, dp, dp * height if dst_chroma_offset is None else dst_chroma_offset, stream)


def scale_device(src, pitch, chroma_offset, width, height, crop, target, out_fmt, dst, lone_field=0, stream=None):
    """jm_amddec_scale_device: crop = (x, y, w, h), target = (tw, th); src / dst device addresses.  Returns 0 or < 0."""
    return lib().jm_amddec_scale_device(src, pitch, chroma_offset, width, height, lone_field, *crop, *target, out_fmt, dst, stream)


# ---- placed output (include/jm_amd_dec.h; INTEGRATION.md "Placed output") ----------
def fit_rect(cw, ch, tw, th, fit=1, sar=(0, 0)):
    """jm_amddec_fit_rect: the letterbox rectangle (x, y, w, h) of a cw x ch picture with sample aspect ratio sar = (num, den) ((0, 0): square
    samples) inside a tw x th target; fit 1 centred, 2 at the top left.  None for invalid arguments."""
    r = (C.c_int * 4)()
    if lib().jm_amddec_fit_rect(cw, ch, sar[0], sar[1], tw, th, fit, r) != 0:
        return None
    return tuple(r)


def scale_rect_device(src, pitch, chroma_offset, width, height, crop, target, out_fmt, dst, rect, fill=-1, lone_field=0, stream=None):
    """jm_amddec_scale_rect_device: scale_device with the picture placed at rect = (x, y, w, h) of the target (w / h 0: to the target's edge) and
    the rest filled (fill -1: Y'CbCr 16, 128, 128, else 0xYYUUVV).  Returns 0 or < 0."""
    return lib().jm_amddec_scale_rect_device(src, pitch, chroma_offset, width, height, lone_field, *crop, *target, out_fmt, dst, stream, *rect, fill)


def rgb_rect_device(src, pitch, chroma_offset, width, height, crop, target, spec, dst, rect, fill=-1, lone_field=0, stream=None):
    """jm_amddec_rgb_rect_device: rgb_device with the picture placed at rect = (x, y, w, h) of the target and the rest filled (fill -1: black, else
    0xRRGGBB).  Returns 0 or < 0."""
    return lib().jm_amddec_rgb_rect_device(src, pitch, chroma_offset, width, height, lone_field, *crop, *target, C.byref(spec), dst, stream, *rect, fill)


# ---- interpolated chroma of the RGB output (include/jm_amd_dec.h; INTEGRATION.md "RGB output") ----------
def chroma_taps(src_len, dst_len, q, max_taps=5):
    """jm_amddec_chroma_taps: the tap table of one chroma axis, src_len chroma samples -> dst_len outputs of the full target with the siting shift q
    (-1, 0, +1), as scale_taps returns it.  None when the ratio or q is invalid."""
    first, w = (C.c_int * max(dst_len, 1))(), (C.c_short * max(dst_len * max_taps, 1))()
    taps = lib().jm_amddec_chroma_taps(src_len, dst_len, q, first, w, max_taps)
    if taps < 0:
        return None
    return list(first[:dst_len]), [list(w[j * max_taps:j * max_taps + taps]) for j in range(dst_len)]


def rgb_chroma_device(src, pitch, chroma_offset, width, height, crop, target, spec, dst, chroma_loc, rect=(0, 0, 0, 0), fill=-1, lone_field=0, stream=None):
    """jm_amddec_rgb_chroma_device: rgb_rect_device with chroma interpolated to full resolution at chroma_sample_loc_type chroma_loc (0..5).
    Returns 0 or < 0."""
    return lib().jm_amddec_rgb_chroma_device(src, pitch, chroma_offset, width, height, lone_field, *crop, *target, C.byref(spec), dst, stream, *rect, fill,
                                             chroma_loc)


# ---- picture hash (include/jm_amd_dec.h; both hashes are defined in INTEGRATION.md "Picture hash") ----------
def picture_hash_device(src, pitch, chroma_offset, width, height, stream=None):
    """jm_amddec_picture_hash_device: the CRC and the checksum of the decoded picture hash SEI (H.265 D.3.19) of one pitch-linear NV12 surface in
    device memory, per component.  Returns (rc, [crc Y, Cb, Cr], [checksum Y, Cb, Cr]); rc 0 or < 0."""
    crc, chk = (C.c_uint * 3)(), (C.c_uint * 3)()
    rc = lib().jm_amddec_picture_hash_device(src, pitch, chroma_offset, width, height, crc, chk, stream)
    return rc, list(crc), list(chk)


def picture_md5_device(src, pitch, chroma_offset, width, height, stream=None):
    """jm_amddec_picture_md5_device: the MD5 (RFC 1321; hash_type 0 of the same SEI message) of each component of one pitch-linear NV12 surface in
    device memory.  Returns (rc, [digest of Y, Cb, Cr: 16 bytes each]); rc 0 or < 0."""
    md5 = ((C.c_ubyte * 16) * 3)()
    rc = lib().jm_amddec_picture_md5_device(src, pitch, chroma_offset, width, height, md5, stream)
    return rc, [bytes(md5[c]) for c in range(3)]


# ---- RGB output (include/jm_amd_dec.h; the conversion C is defined in INTEGRATION.md "RGB output") ----------
class RgbSpec(C.Structure):
    """jm_amddec_rgb_spec."""
    _fields_ = [("dtype", C.c_int), ("planar", C.c_int), ("bgr", C.c_int), ("matrix", C.c_int), ("range", C.c_int),
                ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


RGB_DTYPES = {"u8": 0, "f32": 1, "f16": 2, "bf16": 3}
RGB_SAMPLE_BYTES = {0: 1, 1: 4, 2: 2, 3: 2}


def rgb_spec(dtype="f16", planar=True, bgr=False, matrix=0, range=0, mean=None, std=None, scale=None, bias=None):
    """An RgbSpec.  dtype: "u8" / "f32" / "f16" / "bf16" (or 0..3).  scale / bias per storage position; mean / std (per storage position, on the
    0..1 scale) give the normalisation scale = 1 / (255 std), bias = -mean / std.  Without any of them: scale 1, bias 0 (floats in [0, 255])."""
    s = RgbSpec()
    s.dtype = RGB_DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    s.planar, s.bgr, s.matrix, s.range = int(bool(planar)), int(bool(bgr)), int(matrix), int(range)
    sc, bi = [1.0] * 3, [0.0] * 3
    if mean is not None or std is not None:
        m = list(mean) if mean is not None else [0.0] * 3
        d = list(std) if std is not None else [1.0] * 3
        sc = [1.0 / (255.0 * d[c]) for c in (0, 1, 2)]
        bi = [-m[c] / d[c] for c in (0, 1, 2)]
    if scale is not None:
        sc = list(scale)
    if bias is not None:
        bi = list(bias)
    for c in (0, 1, 2):
        s.scale[c], s.bias[c] = sc[c], bi[c]
    return s


def set_rgb(handle, dtype="f16", planar=True, bgr=False, matrix=0, range=0, mean=None, std=None, scale=None, bias=None):
    """jm_amddec_set_rgb before init (the arguments as rgb_spec; an RgbSpec as dtype is used as it is; dtype=None: Y'CbCr output again).
    Returns 0 or -1."""
    if dtype is None:
        return lib().jm_amddec_set_rgb(handle, None)
    s = dtype if isinstance(dtype, RgbSpec) else rgb_spec(dtype, planar, bgr, matrix, range, mean, std, scale, bias)
    return lib().jm_amddec_set_rgb(handle, C.byref(s))


def color_coefs(matrix, full_range):
    """jm_amddec_color_coefs: (cy, crv, cgu, cgv, cbu), or None when the matrix is not supported."""
    c = (C.c_int * 5)()
    return tuple(c) if lib().jm_amddec_color_coefs(matrix, int(full_range), c) == 0 else None


def rgb_device(src, pitch, chroma_offset, width, height, crop, target, spec, dst, lone_field=0, stream=None):
    """jm_amddec_rgb_device: crop = (x, y, w, h), target = (tw, th), spec an RgbSpec with an explicit matrix; src / dst device addresses.
    Returns 0 or < 0."""
    return lib().jm_amddec_rgb_device(src, pitch, chroma_offset, width, height, lone_field, *crop, *target, C.byref(spec), dst, stream)


def bf16_to_f32(bits):
    """bf16 samples (uint16 bit patterns, as rgb_array returns them) as float32."""
    import numpy as np
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def rgb_array(buf, w, h, spec):
    """An RGB frame (bytes) as a numpy array: (3, h, w) planar or (h, w, 3) interleaved; u8 / float32 / float16, bf16 as uint16 bit patterns."""
    import numpy as np
    dt = {0: np.uint8, 1: np.float32, 2: np.float16, 3: np.uint16}[spec.dtype]
    a = np.frombuffer(bytes(buf), dtype=dt, count=3 * w * h)
    return a.reshape((3, h, w) if spec.planar else (h, w, 3))


# ---- the reference harness's NAL scanner (test_nv_dec.cpp:30-86), vectorised -----------------
def split_nalus(data):
    """Split an Annex-B buffer into chunks exactly as test_nv_dec's find_nalu does: each chunk
    starts at a start code (00 00 01 or 00 00 00 01) and runs up to the next one."""
    import numpy as np
    a = np.frombuffer(data, dtype=np.uint8)
    if len(a) < 4:
        return [bytes(data)]
    m = (a[:-2] == 0) & (a[1:-1] == 0) & (a[2:] == 1)
    idx = np.flatnonzero(m)
    starts = []
    for i in idx:
        s = int(i)
        if s > 0 and a[s - 1] == 0:
            s -= 1                      # 4-byte start code: find_nalu_prefix matches it one byte earlier
        if not starts or s > starts[-1]:
            starts.append(s)
    out = []
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(a)
        out.append(bytes(data[s:e]))
    return out


def split_jpegs(data):
    """Split a byte stream of concatenated JPEG pictures (MJPEG, codec_type 2) into one chunk per picture, SOI .. EOI.  Segments are walked by their
    length fields, so an APPn segment that embeds a thumbnail's SOI / EOI stays inside its picture; entropy-coded data ends at the first marker that
    is neither a stuffed FF 00 nor RSTn.  Bytes between pictures go with the picture in front of them; a last picture without EOI is its own chunk.
    (The decoder itself accepts any chunking: this is a convenience for callers that want one picture per call.)"""
    data = bytes(data)
    n, cuts, o = len(data), [], data.find(b"\xff\xd8")
    while 0 <= o < n:
        cuts.append(o)
        o += 2
        while o < n:                                        # one picture: marker segments, then entropy-coded data, until EOI
            if data[o] != 0xFF:
                o += 1
                continue
            while o < n and data[o] == 0xFF:
                o += 1
            if o >= n:
                break
            m = data[o]
            o += 1
            if m == 0xD9:
                break
            if m == 0xD8:                                   # a picture that never ended
                o -= 2
                break
            if m == 0 or m == 1 or 0xD0 <= m <= 0xD7 or o + 2 > n:
                continue
            ln = data[o] << 8 | data[o + 1]
            if ln < 2:
                continue
            o += ln
            if m == 0xDA:
                while o < n:
                    o = data.find(b"\xff", o)
                    if o < 0 or o + 1 >= n:
                        o = n
                    elif data[o + 1] == 0 or 0xD0 <= data[o + 1] <= 0xD7:
                        o += 2
                        continue
                    break
        o = data.find(b"\xff\xd8", o)
    if not cuts:
        return [data] if data else []
    cuts[0] = 0
    return [data[a:b] for a, b in zip(cuts, cuts[1:] + [n])]


def split_mpeg2_pictures(data):
    """Split an MPEG-2 video elementary stream (codec_type 4) into one chunk per picture: a chunk starts at the first sequence header, group header or
    picture header that follows a slice (or the sequence end code), so the headers in front of a picture travel with it; what precedes the first
    such start code goes with the first picture.  (The decoder itself accepts any chunking: this is a convenience for callers that want one picture
    per call.)"""
    data = bytes(data)
    cuts, after_slice, o = [0], False, data.find(b"\x00\x00\x01")
    while 0 <= o and o + 3 < len(data):
        code = data[o + 3]
        if code in (0x00, 0xB3, 0xB8) and after_slice:
            cuts.append(o)
            after_slice = False
        elif 0x01 <= code <= 0xAF or code == 0xB7:
            after_slice = True
        o = data.find(b"\x00\x00\x01", o + 3)
    return [data[a:b] for a, b in zip(cuts, cuts[1:] + [len(data)])] if data else []


def webp_to_ivf(data):
    """The `VP8 ` chunk of a lossy RIFF / WebP file as a one-frame IVF byte stream for a codec_type 5 handle (the library itself parses no RIFF wrapper).
    Raises ValueError for a file without such a chunk (lossless `VP8L`, or no WebP at all); an `ALPH` chunk is ignored."""
    data = bytes(data)
    if data[:4] != b"RIFF" or data[8:12] != b"WEBP":
        raise ValueError("not a RIFF / WebP file")
    o = 12
    while o + 8 <= len(data):
        n = int.from_bytes(data[o + 4:o + 8], "little")
        if data[o:o + 4] == b"VP8 ":
            f = data[o + 8:o + 8 + n]
            head = b"DKIF" + (0).to_bytes(2, "little") + (32).to_bytes(2, "little") + b"VP80" + bytes(4) + (30).to_bytes(4, "little") + \
                (1).to_bytes(4, "little") + (1).to_bytes(4, "little") + bytes(4)
            return head + len(f).to_bytes(4, "little") + bytes(8) + f
        o += 8 + n + (n & 1)
    raise ValueError("no VP8 chunk (a lossless or animated WebP file?)")


def annexb_to_avcc(data, length_size=4):
    """(avcC record, [length-prefixed packets]) of an Annex-B stream: what a demuxer hands test_player for an MP4 source when no
    h264_mp4toannexb filter is in the way (test_player.cpp:221-226).  One packet per access unit (split before each first slice)."""
    nalus = [n.lstrip(b"\x00")[1:] for n in split_nalus(data)]              # strip start codes
    sps = [n for n in nalus if n and (n[0] & 31) == 7]
    pps = [n for n in nalus if n and (n[0] & 31) == 8]
    rec = bytes([1, sps[0][1], sps[0][2], sps[0][3], 0xFC | (length_size - 1), 0xE0 | 1]) + len(sps[0]).to_bytes(2, "big") + sps[0]
    rec += bytes([1]) + len(pps[0]).to_bytes(2, "big") + pps[0]
    packets, cur = [], b""
    for n in nalus:
        t = n[0] & 31
        if t in (7, 8):
            continue
        if t in (1, 5) and (n[1] & 0x80) and cur:                            # first_mb_in_slice == 0: a new picture starts
            packets.append(cur)
            cur = b""
        cur += len(n).to_bytes(length_size, "big") + n
    if cur:
        packets.append(cur)
    return rec, packets


def annexb_to_hvcc(data, length_size=4):
    """(hvcC record, [length-prefixed packets]) of an HEVC Annex-B stream: the MP4 / MKV form of the same stream (one packet per access
    unit, parameter sets only in the record)."""
    nalus = [n.lstrip(b"\x00")[1:] for n in split_nalus(data)]
    ps = {32: [], 33: [], 34: []}
    for n in nalus:
        t = (n[0] >> 1) & 63
        if t in ps and n not in ps[t]:
            ps[t].append(n)
    rec = bytes([1]) + bytes(20) + bytes([0xFC | (length_size - 1), sum(1 for t in ps if ps[t])])
    for t in (32, 33, 34):
        if ps[t]:
            rec += bytes([0x80 | t]) + len(ps[t]).to_bytes(2, "big") + b"".join(len(n).to_bytes(2, "big") + n for n in ps[t])
    packets, cur = [], b""
    for n in nalus:
        t = (n[0] >> 1) & 63
        if t in ps:
            continue
        if (t <= 9 or 16 <= t <= 21) and (n[2] & 0x80) and cur:            # first_slice_segment_in_pic_flag: a new picture starts
            packets.append(cur)
            cur = b""
        cur += len(n).to_bytes(length_size, "big") + n
    if cur:
        packets.append(cur)
    return rec, packets


class JmAmdDec:
    """Convenience wrapper reproducing test_nv_dec's main loop (test_nv_dec.cpp:163-259).

    codec_type: 0 H.264, 1 HEVC, 2 MJPEG, 4 MPEG-2 video (frame pictures, 4:2:0: INTEGRATION.md "MPEG-2"), 5 VP8 key frames (needs options={"vp8": 1}; an IVF byte
    stream in any chunking or one frame per call: INTEGRATION.md "VP8"; `webp_to_ivf` wraps a lossy WebP file; options={"vp8": 1, "vp8_inter": 1} decodes inter frames too --
    golden / altref references, motion vectors, six-tap and bilinear prediction; without "vp8_inter" an inter frame fails the handle, and the option is
    refused for every other codec_type and without "vp8"; stats vp8_inter_frames, vp8_golden_refs, vp8_altref_refs, vp8_split_mbs,
    vp8_intra_in_inter_mbs); the other values of the reference's NV_CODEC_TYPE are refused at init."""

    def __init__(self, codec_type=0, out_fmt=1, options=None, extra_data=None, rgb=None):
        self.h = jm_nvdec_create_handle()
        for k, v in (options or {}).items():
            lib().jm_amddec_set_option(self.h, k.encode(), int(v))
        # rgb: an RgbSpec, or a dict of set_rgb's keyword arguments -- frames then leave as RGB (rgb_array turns them into arrays)
        if rgb is not None and (set_rgb(self.h, rgb) if isinstance(rgb, RgbSpec) else set_rgb(self.h, **rgb)) != 0:
            jm_nvdec_deinit(self.h)
            self.h = None
            raise ValueError("invalid RGB spec")
        rc = jm_nvdec_init(codec_type, out_fmt, extra_data, len(extra_data) if extra_data else 0, self.h)
        if rc != 0:
            err = lib().jm_amddec_last_error(self.h).decode()
            jm_nvdec_deinit(self.h)
            self.h = None
            raise RuntimeError(f"jm_nvdec_init failed: {err}")
        self.out_buf = None
        self.nalu_count = 0

    def stat(self, key):
        return lib().jm_amddec_get_stat(self.h, key.encode())

    def _pull(self, frames):
        need = self.stat("out_frame_bytes")                    # bytes of the frame about to be fetched (it can change at an IDR picture)
        if self.out_buf is None or len(self.out_buf) < need:
            self.out_buf = C.create_string_buffer(max(need, 16))
        ret, n = jm_nvdec_output_frame(self.out_buf, len(self.out_buf), self.h)
        if n > 0 and frames is not None:
            frames.append(self.out_buf.raw[:n])
        return n > 0

    def decode_stream(self, data, keep=True, chunks=None):
        """Feed one NAL per call, then drain with (NULL, 0) until is_exit.  Returns list of frames
        (bytes) when keep, else the frame count."""
        frames = [] if keep else None
        count = 0
        for nal in (chunks if chunks is not None else split_nalus(data)):
            self.nalu_count += 1
            _, got = jm_nvdec_decode_frame(nal, len(nal), self.h)
            if got == 1 and self._pull(frames):
                count += 1
        while not jm_nvdec_is_exit(self.h):
            self.nalu_count += 1
            ret, got = jm_nvdec_decode_frame(None, 0, self.h)
            if ret != 0:
                raise RuntimeError(lib().jm_amddec_last_error(self.h).decode())
            if got == 1 and self._pull(frames):
                count += 1
        return frames if keep else count

    def close(self):
        if self.h:
            jm_nvdec_deinit(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ---- the reference's push / pull API (intel_dec/jm_intel_dec.h:29-122), same names and argument order ----
YUV_CALLBACK = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_void_p)     # HANDLE_YUV_CALLBACK, jm_intel_dec.h:20


def jm_intel_is_hw_support():
    return bool(lib().jm_amdintel_is_hw_support())


def jm_intel_dec_create_handle():
    return lib().jm_amdintel_create_handle()


def jm_intel_dec_init(codec_type, out_fmt, handle):
    return lib().jm_amdintel_init(codec_type, out_fmt, handle)


def jm_intel_dec_deinit(handle):
    return lib().jm_amdintel_deinit(handle)


def jm_intel_dec_set_yuv_callback(user_data, callback, handle):
    """callback: a YUV_CALLBACK instance (the caller keeps it alive) or None."""
    return lib().jm_amdintel_set_yuv_callback(user_data, C.cast(callback, C.c_void_p) if callback else None, handle)


def jm_intel_dec_input_data(in_buf, in_data_len, handle):
    """in_buf: bytes or a ctypes buffer / address.  Returns the bytes accepted (> 0) or < 0."""
    if isinstance(in_buf, (bytes, bytearray)):
        in_buf = C.cast(C.c_char_p(bytes(in_buf)), C.c_void_p)
    return lib().jm_amdintel_input_data(in_buf, in_data_len, handle)


def jm_intel_dec_output_frame(out_buf, out_len, handle):
    """out_buf: writable ctypes buffer or None (size query); out_len: its capacity.  Returns (ret, bytes): ret 0 = a frame was copied,
    -1 = none ready, -2 = buffer too small (jm_intel_dec.h:69-78)."""
    n = C.c_int(out_len)
    ret = lib().jm_amdintel_output_frame(C.cast(out_buf, C.c_void_p) if out_buf is not None else None, C.byref(n), handle)
    return ret, n.value


def jm_intel_dec_set_eof(is_eof, handle):
    return lib().jm_amdintel_set_eof(int(is_eof), handle)


def jm_intel_dec_info(handle):
    s = lib().jm_amdintel_info(handle)
    return s.decode() if s else ""


def jm_intel_get_stream_info(handle):
    """Returns (ret, width, height, frame_rate)."""
    w, h, f = C.c_int(0), C.c_int(0), C.c_float(0.0)
    ret = lib().jm_amdintel_get_stream_info(C.byref(w), C.byref(h), C.byref(f), handle)
    return ret, w.value, h.value, f.value


def jm_intel_dec_need_more_data(handle):
    return bool(lib().jm_amdintel_need_more_data(handle))


def jm_intel_dec_free_buf_len(handle):
    return lib().jm_amdintel_free_buf_len(handle)


def jm_intel_dec_is_exit(handle):
    return bool(lib().jm_amdintel_is_exit(handle))


def intel_push_pull(data, codec_type=0, out_fmt=1, callback=False, max_push=None, on_frame=None, options=None):
    """The loop of /root/reference/test_intel_dec/test_intel_dec.cpp:64-102 over an Annex-B buffer: while not is_exit: if need_more_data and input is
    left, input_data(min(free_buf_len, remaining)) -- set_eof when it ran out; then one output_frame.  Frames go to ``on_frame(bytes)`` (default: a
    list that is returned), through output_frame or -- callback=True -- through the YUV callback.  Returns (frames, info string, stream info tuple,
    largest single push)."""
    frames = []
    sink = on_frame or frames.append
    cb = YUV_CALLBACK(lambda p, n, u: sink(C.string_at(p, n)) or 0)
    h = jm_intel_dec_create_handle()
    for k, v in (options or {}).items():
        lib().jm_amddec_set_option(lib().jm_amdintel_decoder(h), k.encode(), int(v))
    if jm_intel_dec_init(codec_type, out_fmt, h) != 0:
        jm_intel_dec_deinit(h)
        raise RuntimeError("jm_intel_dec_init failed")
    try:
        if callback:
            jm_intel_dec_set_yuv_callback(None, cb, h)
        data = bytes(data)
        mv = memoryview(data)
        base = C.cast(C.c_char_p(data), C.c_void_p).value
        out = C.create_string_buffer(20 << 20)                       # the harness's 20 MB output buffer, test_intel_dec.cpp:50
        pos, is_eof, biggest, guard, sinfo = 0, False, 0, 0, None
        while not jm_intel_dec_is_exit(h):
            guard += 1
            if guard > 50_000_000:
                raise RuntimeError("push / pull loop does not terminate")
            if jm_intel_dec_need_more_data(h) and not is_eof:
                k = min(jm_intel_dec_free_buf_len(h), len(mv) - pos)
                if max_push:
                    k = min(k, max_push)
                if k == 0:
                    is_eof = True
                    jm_intel_dec_set_eof(1, h)
                else:
                    if jm_intel_dec_input_data(base + pos, k, h) != k:
                        raise RuntimeError("jm_intel_dec_input_data failed")
                    pos += k
                    biggest = max(biggest, k)
            ret, n = jm_intel_dec_output_frame(out, len(out), h)
            if ret == 0:
                if callback:
                    raise RuntimeError("output_frame handed out a frame although a callback is set")
                sink(C.string_at(out, n))
                if sinfo is None:
                    sinfo = jm_intel_get_stream_info(h)
        if sinfo is None:
            sinfo = jm_intel_get_stream_info(h)
        if lib().jm_amddec_get_stat(lib().jm_amdintel_decoder(h), b"failed") == 1:
            raise RuntimeError(lib().jm_amddec_last_error(lib().jm_amdintel_decoder(h)).decode())
        return frames, jm_intel_dec_info(h), sinfo, biggest
    finally:
        jm_intel_dec_deinit(h)
