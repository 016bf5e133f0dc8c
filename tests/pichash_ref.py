"""Reference for the decoded picture hash SEI (H.265 D.3.19; INTEGRATION.md "Picture hash") -- a helper, not a test.  Nothing here calls the product:
the checksum is the formula in numpy, the CRC is the bit-serial loop (and binascii's CRC-CCITT for speed, which test_pichash_host.py shows to be the
same function), the SEI payload is assembled byte by byte."""
import binascii
import ctypes as C
import hashlib

import numpy as np

MD5, CRC, CHECKSUM = 0, 1, 2


def checksum(plane):
    """sum over (y, x) of s[y][x] ^ ((x & 255) ^ (y & 255) ^ (x >> 8) ^ (y >> 8)), mod 2^32; x, y the component's own coordinates."""
    p = np.asarray(plane, dtype=np.uint8)
    h, w = p.shape
    x, y = np.arange(w, dtype=np.uint32)[None, :], np.arange(h, dtype=np.uint32)[:, None]
    m = (x & 255) ^ (y & 255) ^ (x >> 8) ^ (y >> 8)
    return int((p.astype(np.uint32) ^ m).sum(dtype=np.uint64) & 0xFFFFFFFF)


def crc_bit_serial(data):
    """crc = 0xFFFF; 16 zero bits appended; per bit, MSB first: crc = ((crc << 1) + bit) & 0xFFFF, xor 0x1021 if the old bit 15 was set."""
    crc = 0xFFFF
    for v in bytes(data) + b"\x00\x00":
        for k in range(7, -1, -1):
            msb = crc & 0x8000
            crc = ((crc << 1) + ((v >> k) & 1)) & 0xFFFF
            if msb:
                crc ^= 0x1021
    return crc


def crc(plane):
    """The same value through binascii (CRC-CCITT, direct form, initial value 0x1D0F)."""
    return binascii.crc_hqx(np.ascontiguousarray(plane, dtype=np.uint8).tobytes(), 0x1D0F)


def md5(plane):
    return hashlib.md5(np.ascontiguousarray(plane, dtype=np.uint8).tobytes()).digest()


def picture_hash(planes, hash_type):
    """[value of Y, Cb, Cr]: ints for CRC / checksum, 16 bytes each for MD5."""
    f = {MD5: md5, CRC: crc, CHECKSUM: checksum}[hash_type]
    return [f(p) for p in planes]


def sei_payload(hash_type, values):
    """The payload of a decoded picture hash message (type 132) of a 4:2:0 picture: hash_type u(8), then per component 16 bytes / u(16) / u(32)."""
    out = bytes([hash_type])
    for v in values:
        out += bytes(v) if hash_type == MD5 else int(v).to_bytes(2 if hash_type == CRC else 4, "big")
    return out


def surface(planes, pitch, pad_rows=0, poison=0xA5):
    """An NV12 surface holding the three planes: (bytes as a uint8 array, chroma_offset).  Everything that is not a sample is `poison`."""
    Y, Cb, Cr = (np.asarray(p, dtype=np.uint8) for p in planes)
    h, w = Y.shape
    rows = h + pad_rows
    s = np.full((rows + h // 2, pitch), poison, dtype=np.uint8)
    s[:h, :w] = Y
    s[rows:, 0:w:2] = Cb
    s[rows:, 1:w:2] = Cr
    return s.reshape(-1), rows * pitch


def frames_to_planes(frames, w, h):
    """Tight I420 frames (bytes) -> [(Y, Cb, Cr)]."""
    out = []
    for f in frames:
        a = np.frombuffer(f, dtype=np.uint8)
        out.append((a[:w * h].reshape(h, w), a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), a[w * h * 5 // 4:].reshape(h // 2, w // 2)))
    return out


def oracle_pictures(data):
    """The CPU oracle's pictures of an HEVC stream in DECODE order: ([(Y, Cb, Cr)], [POC]).  Cropped to the conformance window, so only streams whose
    coded size is their display size give the planes the hash covers."""
    from tools import streams
    orc = streams.OracleHevc()

    class Frame(C.Structure):
        _fields_ = [("y", C.POINTER(C.c_ubyte)), ("u", C.POINTER(C.c_ubyte)), ("v", C.POINTER(C.c_ubyte)), ("width", C.c_int), ("height", C.c_int),
                    ("stride_y", C.c_int), ("stride_c", C.c_int), ("poc", C.c_int), ("slice_type", C.c_int), ("decode_index", C.c_int)]
    got = {}

    def plane(p, w, h, stride):
        a = np.ctypeslib.as_array(p, shape=(h * stride,))[:(h - 1) * stride + w]
        return np.array([a[r * stride:r * stride + w] for r in range(h)], dtype=np.uint8)

    def on_frame(user, fp):
        f = fp.contents
        got[f.decode_index] = ((plane(f.y, f.width, f.height, f.stride_y), plane(f.u, f.width // 2, f.height // 2, f.stride_c),
                                plane(f.v, f.width // 2, f.height // 2, f.stride_c)), f.poc)
    cb = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(Frame))(on_frame)
    d = orc.L.orch_open(C.cast(cb, C.c_void_p), None)
    rc = orc.L.orch_decode_annexb(d, data, len(data))
    orc.L.orch_flush(d)
    orc.L.orch_close(d)
    assert rc >= 0 and sorted(got) == list(range(len(got))), "oracle: not every decoded picture was handed out"
    return [got[k][0] for k in sorted(got)], [got[k][1] for k in sorted(got)]
