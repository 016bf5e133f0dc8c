// jmcodec_amd/csrc/hevc_sei.h -- the one SEI message the decoder reads: decoded picture hash (payload type 132, H.265 D.2.19 / D.3.19) in a suffix
// SEI NAL unit (type 40).  Host only, option verify_hash.  The reference never sees SEI: cuvidParseVideoData takes the bytes
// (/root/reference/nv_dec/nv_dec.cpp:368-403).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace jmamd {

struct HevcPicHash {
    int type = -1;                 // hash_type: 0 MD5, 1 CRC, 2 checksum; -1 = the picture carries none
    uint32_t v[3] = {0, 0, 0};     // Y, Cb, Cr of a CRC (16 bits) or a checksum
    uint8_t md5[3][16] = {};       // Y, Cb, Cr of an MD5: the 16 bytes as MD5 emits them (RFC 1321 order), compared with option verify_md5
};

// Walks every sei_message of an unescaped SEI RBSP (the bytes behind the two-byte NAL header).  A type-132 message of 4:2:0 content (three
// components) with a known hash_type lands in `out` (a later one replaces an earlier one) and sets `found`.  Returns the number of malformed
// messages: one that runs past the buffer, or a type-132 message whose size is not what its hash_type needs -- such a message is ignored, and the walk
// ends at a message whose size cannot be trusted.  Reads rbsp[0 .. n - 1] only.
int parse_sei_picture_hash(const uint8_t *rbsp, size_t n, HevcPicHash &out, bool &found);

}  // namespace jmamd
