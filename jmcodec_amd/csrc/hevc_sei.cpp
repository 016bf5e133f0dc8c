// jmcodec_amd/csrc/hevc_sei.cpp -- see hevc_sei.h.  The syntax is written from memory of H.265 7.3.5 (sei_message: 0xFF-extended payload type and size
// bytes) and D.2.19 (hash_type u(8), then per component 16 bytes, u(16) or u(32)): no copy of the standard is at hand.
#include "hevc_sei.h"
#include <string.h>

namespace jmamd {

int parse_sei_picture_hash(const uint8_t *b, size_t n, HevcPicHash &out, bool &found) {
    int bad = 0;
    // rbsp_trailing_bits: every sei_message ends byte aligned, so the stop bit is a byte of its own
    size_t end = n;
    if (end > 0 && b[end - 1] == 0x80) end--;
    size_t pos = 0;
    while (pos < end) {
        unsigned type = 0, size = 0;
        while (pos < end && b[pos] == 0xFF && type < (1u << 20)) { type += 255; pos++; }
        if (pos >= end || b[pos] == 0xFF) return bad + 1;
        type += b[pos++];
        while (pos < end && b[pos] == 0xFF && size < (1u << 20)) { size += 255; pos++; }
        if (pos >= end || b[pos] == 0xFF) return bad + 1;
        size += b[pos++];
        if (size > end - pos) return bad + 1;                      // truncated: nothing behind it can be trusted either
        if (type == 132) {
            const uint8_t *p = b + pos;
            const int ht = size >= 1 ? p[0] : -1;
            const unsigned need = ht == 0 ? 48 : (ht == 1 ? 6 : (ht == 2 ? 12 : 0));
            if (ht < 0 || (ht <= 2 && size - 1 != need)) bad++;     // (hash_type 3 .. 255 is reserved: skipped like an unknown payload)
            else if (ht <= 2) {
                HevcPicHash h;
                h.type = ht;
                for (int c = 0; c < 3 && ht == 0; c++) memcpy(h.md5[c], p + 1 + 16 * c, 16);       // (size - 1 == 48 was checked)
                for (int c = 0; c < 3 && ht > 0; c++) {
                    const uint8_t *q = p + 1 + (ht == 1 ? 2 : 4) * c;
                    h.v[c] = ht == 1 ? (uint32_t)q[0] << 8 | q[1] : (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3];
                }
                out = h; found = true;
            }
        }
        pos += size;
    }
    return bad;
}

}  // namespace jmamd
