"""Stamps an HEVC Annex-B stream with decoded picture hash SEI messages (payload type 132 in suffix SEI NAL units, type 40; H.265 D.2.19), the way HM
does by default and x265 does with --hash: what option verify_hash of the decoder checks.  The hashes come from tests/pichash_ref.py -- the formulas
written out in Python -- and from pictures the CALLER supplies (the analytic expectation, the CPU oracle's pictures), never from the product.
tools/hevcgen.c is not involved: the stream is cut at its start codes and the new NAL units are put between the old ones."""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(_ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(_ROOT, "tests"))
import pichash_ref as ref  # noqa: E402


def split_nals(stream):
    """[(start code, NAL bytes)] of an Annex-B stream.  Zero bytes in front of 00 00 01 belong to the start code (a NAL unit never ends in a zero
    byte), and so does whatever precedes the first one: b"".join(sc + nal) is the stream again."""
    stream = bytes(stream)
    marks, i = [], stream.find(b"\x00\x00\x01")
    while i >= 0:
        marks.append(i)
        i = stream.find(b"\x00\x00\x01", i + 3)
    out, begin = [], 0                                      # begin: where the current start code begins
    for k, s in enumerate(marks):
        e = marks[k + 1] if k + 1 < len(marks) else len(stream)
        nal_end = e
        while k + 1 < len(marks) and nal_end > s + 3 and stream[nal_end - 1] == 0:
            nal_end -= 1
        out.append((stream[begin:s + 3], stream[s + 3:nal_end]))
        begin = nal_end
    return out


def nal_type(nal):
    return (nal[0] >> 1) & 63


def is_vcl(nal):
    return nal_type(nal) <= 9 or 16 <= nal_type(nal) <= 21


def escape(rbsp):
    """Emulation prevention: 00 00 0x (x <= 3) becomes 00 00 03 0x."""
    out, zeros = bytearray(), 0
    for b in bytes(rbsp):
        if zeros >= 2 and b <= 3:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def sei_message(payload_type, payload):
    """One sei_message: 0xFF-extended type and size bytes, then the payload."""
    def ext(v):
        return b"\xff" * (v // 255) + bytes([v % 255])
    return ext(payload_type) + ext(len(payload)) + bytes(payload)


def sei_nal(messages, tid_plus1=1, nal_unit_type=40, raw=False):
    """A SEI NAL unit with its start code: two-byte header (layer 0), the messages, rbsp_trailing_bits 0x80, emulation prevention.  raw: `messages` is
    the RBSP as it is (for malformed units: no trailing bits are added)."""
    body = bytes(messages) if raw else bytes(messages) + b"\x80"
    return b"\x00\x00\x01" + bytes([nal_unit_type << 1, tid_plus1 & 7]) + escape(body)


def pictures_of(nals):
    """Per coded picture of the stream, in decode order: (index of its last VCL NAL, nuh_temporal_id_plus1)."""
    pics = []
    for i, (_, nal) in enumerate(nals):
        if not is_vcl(nal):
            continue
        if nal[2] & 0x80 or not pics:                       # first_slice_segment_in_pic_flag
            pics.append([i, nal[1] & 7])
        else:
            pics[-1][0] = i
    return [tuple(p) for p in pics]


def hash_message(planes, hash_type, flip_component=None):
    """The type-132 sei_message of one picture (planes: Y, Cb, Cr as arrays); flip_component: one bit of that component's value is flipped."""
    values = ref.picture_hash(planes, hash_type)
    if flip_component is not None:
        v = values[flip_component]
        values[flip_component] = bytes([v[0] ^ 1]) + v[1:] if hash_type == ref.MD5 else v ^ 1
    return sei_message(132, ref.sei_payload(hash_type, values))


def join(nals, extra):
    """The stream again, with extra[i] (bytes, start codes included) put behind NAL i."""
    return b"".join(sc + nal + extra.get(i, b"") for i, (sc, nal) in enumerate(nals))


def stamp(stream, pictures_in_decode_order, hash_type, corrupt=None):
    """One suffix SEI NAL with the picture's hash behind the last VCL NAL of every picture.  pictures_in_decode_order: [(Y, Cb, Cr)] at the CODED size;
    hash_type 0 MD5, 1 CRC, 2 checksum; corrupt = (k, c): one bit of component c's value of picture k is flipped (the expected value is wrong, the
    slice data is untouched)."""
    nals = split_nals(stream)
    pics = pictures_of(nals)
    if len(pics) != len(pictures_in_decode_order):
        raise ValueError(f"the stream holds {len(pics)} pictures, {len(pictures_in_decode_order)} were supplied")
    extra = {}
    for k, ((last, tid), planes) in enumerate(zip(pics, pictures_in_decode_order)):
        flip = corrupt[1] if corrupt is not None and corrupt[0] == k else None
        extra[last] = sei_nal(hash_message(planes, hash_type, flip), tid)
    return join(nals, extra)
