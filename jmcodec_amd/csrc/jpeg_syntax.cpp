// jmcodec_amd/csrc/jpeg_syntax.cpp -- see jpeg_syntax.h.
#include "jpeg_syntax.h"
#include <algorithm>
#include <cstring>

namespace jmamd {

// T.81 Annex K.3, Tables K.3 - K.6 (tests/test_mjpeg_host.py compares them with the DHT segments libjpeg writes)
const uint8_t kJpegStdDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kJpegStdDcLumaVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kJpegStdDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kJpegStdDcChromaVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kJpegStdAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kJpegStdAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kJpegStdAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kJpegStdAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

bool JpegHuff::build() {
    memset(look, 0, sizeof look);
    int k = 0; uint32_t code = 0;
    for (int l = 1; l <= 16; l++) {
        valoff[l] = k - (int)code;
        for (int i = 0; i < bits[l]; i++, k++, code++) {
            if (k >= 256 || code >= (1u << l)) return false;
            if (l <= 9) { const uint32_t lo = code << (9 - l); for (uint32_t s = 0; s < (1u << (9 - l)); s++) look[lo + s] = (uint16_t)(l << 8 | vals[k]); }
        }
        maxcode[l] = bits[l] ? (int32_t)code - 1 : -1;
        code <<= 1;
    }
    maxcode[17] = 0x7fffffff;
    set = true;
    return true;
}

static void std_table(JpegHuff &h, const uint8_t bits[16], const uint8_t *vals, int n) {
    h = JpegHuff();
    memcpy(h.bits + 1, bits, 16); memcpy(h.vals, vals, (size_t)n);
    h.build();
}

std::string jpeg_parse_picture(const uint8_t *p, size_t n, JpegTables &tab, JpegPic &pic, bool *refuse) {
    auto refused = [&](const char *what) { if (refuse) *refuse = true; return std::string("MJPEG: ") + what + ": not supported"; };
    if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return "MJPEG: the picture does not start with SOI";
    size_t o = 2;
    bool have_sof = false, have_sos = false;
    int adobe = -1;
    struct Comp { int id, h, v, tq, td, ta; } comp[3] = {};
    pic = JpegPic();
    tab.restart_interval = 0;                                   // SOI disables restart intervals (B.2.4.4): only the tables persist
    while (o < n) {
        if (p[o] != 0xFF) { o++; continue; }                    // (bytes between segments: skipped)
        while (o < n && p[o] == 0xFF) o++;                      // fill bytes
        if (o >= n) break;
        const int m = p[o++];
        if (m == 0 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD8) break;                                   // the next picture begins: this one had no EOI
        if (m == 0xD9) break;
        if (o + 2 > n) break;
        const size_t len = (size_t)p[o] << 8 | p[o + 1];
        if (len < 2 || o + len > n) { if (have_sos) break; return "MJPEG: a segment runs past the end of the picture"; }
        const uint8_t *s = p + o + 2; const size_t sl = len - 2;
        o += len;
        if (m == 0xC4) {                                        // DHT
            size_t i = 0;
            while (i < sl) {
                if (i + 17 > sl) return "MJPEG: damaged DHT";
                const int tc = s[i] >> 4, th = s[i] & 15; int cnt = 0;
                if (tc > 1 || th > 3) return "MJPEG: damaged DHT";
                JpegHuff h;
                for (int l = 1; l <= 16; l++) { h.bits[l] = s[i + l]; cnt += s[i + l]; }
                if (cnt > 256 || i + 17 + (size_t)cnt > sl) return "MJPEG: damaged DHT";
                memcpy(h.vals, s + i + 17, (size_t)cnt);
                if (!h.build()) return "MJPEG: a DHT does not describe a prefix code";
                (tc ? tab.ac : tab.dc)[th] = h;
                i += 17 + (size_t)cnt;
            }
        } else if (m == 0xDB) {                                 // DQT
            size_t i = 0;
            while (i < sl) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                if (pq != 0) return refused("16-bit quantisation tables (Pq = 1)");
                if (tq > 3 || i + 65 > sl) return "MJPEG: damaged DQT";
                memcpy(tab.q[tq], s + i + 1, 64); tab.q_set[tq] = true;
                i += 65;
            }
        } else if (m == 0xDD) {                                 // DRI
            if (sl < 2) return "MJPEG: damaged DRI";
            tab.restart_interval = s[0] << 8 | s[1];
        } else if (m == 0xEE) {                                 // APP14: "Adobe", version, flags0, flags1, transform
            if (sl >= 12 && !memcmp(s, "Adobe", 5)) adobe = s[11];
        } else if (m == 0xC0 || m == 0xC1) {                    // SOF0 / SOF1 (extended sequential, Huffman)
            if (have_sof) return "MJPEG: two frame headers in one picture";
            if (sl < 6) return "MJPEG: damaged frame header";
            if (s[0] != 8) return refused(s[0] == 12 ? "12-bit samples" : "a sample precision other than 8 bits");
            pic.height = s[1] << 8 | s[2]; pic.width = s[3] << 8 | s[4]; pic.ncomp = s[5];
            if (pic.height == 0) return refused("a picture height given by DNL");
            if (pic.width == 0) return "MJPEG: damaged frame header";
            if (pic.width > 8192 || pic.height > 8192) return refused("pictures larger than 8192 samples per axis");
            if (pic.ncomp != 1 && pic.ncomp != 3) return refused(pic.ncomp == 4 ? "four components (CMYK / YCCK)" : "a component count other than 1 or 3");
            if (sl < 6 + 3 * (size_t)pic.ncomp) return "MJPEG: damaged frame header";
            for (int c = 0; c < pic.ncomp; c++) { comp[c].id = s[6 + 3 * c]; comp[c].h = s[7 + 3 * c] >> 4; comp[c].v = s[7 + 3 * c] & 15; comp[c].tq = s[8 + 3 * c];
                if (comp[c].tq > 3) return "MJPEG: damaged frame header"; }
            if (pic.ncomp == 1) { pic.sampling = 0x10; comp[0].h = comp[0].v = 1; }      // (one component: its factors do not matter, A.2.2)
            else {
                const int y = comp[0].h << 4 | comp[0].v;
                if (comp[1].h != 1 || comp[1].v != 1 || comp[2].h != 1 || comp[2].v != 1 || (y != 0x22 && y != 0x21 && y != 0x11))
                    return refused("sampling factors other than 4:2:0, 4:2:2 (2x1) and 4:4:4");
                pic.sampling = y;
            }
            have_sof = true;
        } else if (m == 0xC2) return refused("progressive JPEG (SOF2)");
        else if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) return refused("lossless JPEG");
        else if (m == 0xC9 || m == 0xCA || m == 0xCC || m == 0xCD || m == 0xCE) return refused("arithmetic coding");
        else if (m == 0xC5 || m == 0xC6) return refused("hierarchical (differential) JPEG");
        else if (m == 0xDC) return refused("DNL");
        else if (m == 0xDA) {                                   // SOS
            if (have_sos) return refused("several scans in one picture");
            if (!have_sof) return "MJPEG: a scan without a frame header";
            if (sl < 1) return "MJPEG: damaged scan header";
            const int ns = s[0];
            if (ns != pic.ncomp) return refused("several scans in one picture (a scan that does not hold every component)");
            if (sl < 4 + 2 * (size_t)ns) return "MJPEG: damaged scan header";
            for (int c = 0; c < ns; c++) { if (s[1 + 2 * c] != comp[c].id) return "MJPEG: the scan's components do not follow the frame header's";
                comp[c].td = s[2 + 2 * c] >> 4; comp[c].ta = s[2 + 2 * c] & 15;
                if (comp[c].td > 3 || comp[c].ta > 3) return "MJPEG: damaged scan header"; }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return refused("a scan with spectral selection or successive approximation");
            have_sos = true;
            pic.scan_off = o;
            // the entropy-coded data ends at the next marker that is neither a stuffed FF nor RSTn
            size_t e = o;
            for (;;) {
                const uint8_t *f = e < n ? (const uint8_t *)memchr(p + e, 0xFF, n - e) : nullptr;
                if (!f) { e = n; break; }
                e = (size_t)(f - p);
                if (e + 1 >= n) { e = n; break; }
                const int nx = p[e + 1];
                if (nx == 0 || (nx >= 0xD0 && nx <= 0xD7)) { e += 2; continue; }
                if (nx == 0xFF) {                               // fill bytes: a marker follows -- part of the data only in front of RSTn
                    size_t k = e + 1; while (k < n && p[k] == 0xFF) k++;
                    if (k < n && p[k] >= 0xD0 && p[k] <= 0xD7) { e = k + 1; continue; }
                }
                break;
            }
            pic.scan_end = e; o = e;
            // the tables as they are now (a later picture may redefine them while this one waits for its parse thread)
            for (int c = 0; c < pic.ncomp; c++) {
                if (!tab.q_set[comp[c].tq]) return "MJPEG: a quantisation table the picture uses was never defined";
                memcpy(pic.q[c], tab.q[comp[c].tq], 64);
                for (int cls = 0; cls < 2; cls++) {
                    const int id = cls ? comp[c].ta : comp[c].td;
                    const JpegHuff &h = (cls ? tab.ac : tab.dc)[id];
                    JpegHuff &dst = (cls ? pic.ac : pic.dc)[c];
                    if (h.set) dst = h;
                    else if (id > 1) return "MJPEG: a Huffman table the picture uses was never defined";
                    else { pic.used_default_huff = true;       // Annex K.3: table 0 the luminance tables, table 1 the chrominance tables
                        if (!cls) std_table(dst, id ? kJpegStdDcChromaBits : kJpegStdDcLumaBits, id ? kJpegStdDcChromaVals : kJpegStdDcLumaVals, 12);
                        else std_table(dst, id ? kJpegStdAcChromaBits : kJpegStdAcLumaBits, id ? kJpegStdAcChromaVals : kJpegStdAcLumaVals, 162); }
                }
            }
            pic.restart_interval = tab.restart_interval;
        }
        // everything else (APPn, COM, JPGn, ...) is skipped whole by its length: an embedded thumbnail's SOI / EOI is never seen
    }
    if (!have_sof || !have_sos) return "MJPEG: a picture without a frame header and a scan";
    if (adobe >= 0 && adobe != 1) return refused(adobe == 0 ? "an Adobe APP14 transform of 0 (RGB / CMYK samples)" : "an Adobe APP14 transform other than 1");
    const int hs = comp[0].h, vs = comp[0].v;
    pic.mcu_w = 8 * hs; pic.mcu_h = 8 * vs;
    pic.mcus_x = (pic.width + pic.mcu_w - 1) / pic.mcu_w; pic.mcus_y = (pic.height + pic.mcu_h - 1) / pic.mcu_h;
    pic.y_bw = pic.mcus_x * hs; pic.y_bh = pic.mcus_y * vs;
    pic.c_bw = pic.ncomp == 3 ? pic.mcus_x : 0; pic.c_bh = pic.ncomp == 3 ? pic.mcus_y : 0;
    return "";
}

namespace {
struct Bits {
    const uint8_t *p, *end;
    uint64_t acc = 0; int n = 0, fake = 0; bool marker = false;
    void fill() {
        while (n <= 56) {
            if (!marker && n <= 24 && end - p >= 4) {           // four bytes at once when none of them is FF
                uint32_t w; memcpy(&w, p, 4);
                if (!((~w - 0x01010101u) & w & 0x80808080u)) { acc |= (uint64_t)__builtin_bswap32(w) << (32 - n); n += 32; p += 4; continue; }
            }
            unsigned b = 0;
            if (!marker && p < end) {
                b = *p;
                if (b != 0xFF) p++;
                else if (p + 1 < end && p[1] == 0) p += 2;
                else { marker = true; b = 0; fake += 8; }       // a marker (or the end of the data): zeros from here on
            } else { marker = true; fake += 8; }
            acc |= (uint64_t)b << (56 - n); n += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)(acc >> (64 - k)); }
    void skip(int k) { acc <<= k; n -= k; }
    bool overrun() const { return n < fake; }                   // bits that were never in the stream have been consumed
    int decode(const JpegHuff &h) {
        if (n < 16) fill();
        const unsigned e = h.look[peek(9)];
        if (e) { skip((int)(e >> 8)); return (int)(e & 255); }
        const unsigned c16 = peek(16);
        for (int l = 10; l <= 16; l++) { const int c = (int)(c16 >> (16 - l)); if (c <= h.maxcode[l]) { skip(l); return h.vals[(h.valoff[l] + c) & 255]; } }
        return -1;
    }
    int receive_extend(int s) {
        if (n < s) fill();
        const int v = (int)peek(s); skip(s);
        return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    }
};
}  // namespace

std::string jpeg_decode_scan(const JpegPic &pic, const uint8_t *data, size_t n, JpegJobs &jobs) {
    const size_t n_blocks = (size_t)pic.n_blocks();
    jobs.first.assign(n_blocks, 0); jobs.count.assign(n_blocks, 0); jobs.entries.clear();
    if (pic.scan_off > n || pic.scan_end > n || pic.scan_off > pic.scan_end) return "MJPEG: no entropy-coded data";
    Bits br{data + pic.scan_off, data + pic.scan_end};
    long long pred[3] = {0, 0, 0};
    const int hs = pic.mcu_w / 8, vs = pic.mcu_h / 8;
    const size_t nY = (size_t)pic.y_bw * pic.y_bh, nC = (size_t)pic.c_bw * pic.c_bh;
    const int blocks_per_mcu = pic.ncomp == 3 ? hs * vs + 2 : 1;
    long long mcu = 0;
    for (int my = 0; my < pic.mcus_y; my++) for (int mx = 0; mx < pic.mcus_x; mx++, mcu++) {
        if (pic.restart_interval && mcu && mcu % pic.restart_interval == 0) {
            // RSTn: the rest of the byte is padding; fill bytes may precede the marker; any index is accepted; the predictors start again
            if (br.overrun()) return "MJPEG: the entropy-coded data ends early (damaged or truncated picture)";
            if (!br.marker) br.fill();
            if (!br.marker || br.n - br.fake >= 8) return "MJPEG: a restart marker is missing";
            const uint8_t *q = br.p;
            while (q < br.end && *q == 0xFF) q++;
            if (q == br.p || q >= br.end || *q < 0xD0 || *q > 0xD7) return "MJPEG: a restart marker is missing";
            br = Bits{q + 1, br.end};
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int b = 0; b < blocks_per_mcu; b++) {
            int c; size_t idx;
            if (b < hs * vs || pic.ncomp == 1) { c = 0; idx = (size_t)(my * vs + b / hs) * pic.y_bw + (size_t)(mx * hs + b % hs); }
            else { c = b - hs * vs + 1; idx = nY + (size_t)(c - 1) * nC + (size_t)my * pic.c_bw + mx; }
            jobs.first[idx] = (uint32_t)jobs.entries.size();
            auto put = [&](int k, long long level) {
                const int lv = level < -32768 ? -32768 : (level > 32767 ? 32767 : (int)level);      // (leaves clip(level * Q) unchanged: jpeg_jobs.h)
                jobs.entries.push_back((uint32_t)k | (uint32_t)(uint16_t)lv << 16);
            };
            int s = br.decode(pic.dc[c]);
            if (s < 0 || s > 15) { jobs.entries.resize(jobs.first[idx]); return "MJPEG: an invalid Huffman code (damaged picture)"; }
            if (s) pred[c] += br.receive_extend(s);
            if (pred[c]) put(0, pred[c]);
            bool bad = false;
            for (int k = 1; k < 64;) {
                const int rs = br.decode(pic.ac[c]);
                if (rs < 0) { bad = true; break; }
                const int r = rs >> 4; s = rs & 15;
                if (s == 0) { if (r == 15) { k += 16; continue; } break; }      // ZRL; EOB
                k += r;
                if (k > 63) { bad = true; break; }
                put(k, br.receive_extend(s));
                k++;
            }
            if (bad || br.overrun()) {                          // the block that met the damage stays empty, like every block behind it
                jobs.entries.resize(jobs.first[idx]);
                return bad ? "MJPEG: an invalid Huffman code (damaged picture)" : "MJPEG: the entropy-coded data ends early (damaged or truncated picture)";
            }
            jobs.count[idx] = (uint8_t)(jobs.entries.size() - jobs.first[idx]);
        }
    }
    return "";
}

std::string jpeg_segment_scan(const JpegPic &pic, const uint8_t *data, size_t n, JpegSegments &out) {
    out.segs.clear(); out.bytes.clear(); out.n_entries = 0;
    const long long mcus = (long long)pic.mcus_x * pic.mcus_y, want = jpeg_expected_segments(pic);
    const uint32_t bpm = pic.ncomp == 3 ? (uint32_t)(pic.mcu_w / 8) * (uint32_t)(pic.mcu_h / 8) + 2 : 1;
    const long long per = pic.restart_interval > 0 ? pic.restart_interval : mcus;
    std::string err;
    size_t o = pic.scan_off, end = pic.scan_end;
    if (o > n || end > n || o > end) { o = end = 0; err = "MJPEG: no entropy-coded data"; }
    out.bytes.reserve(end - o + (size_t)want * (3 + kJpegSegGuard));
    bool data_left = true;
    for (long long i = 0; i < want; i++) {
        JpegSegment sg;
        sg.byte_off = (uint32_t)out.bytes.size();
        sg.first_mcu = (uint32_t)(i * per); sg.n_mcus = (uint32_t)std::min(per, mcus - i * per);
        bool at_rst = false;
        while (data_left && o < end) {
            const uint8_t *f = (const uint8_t *)memchr(data + o, 0xFF, end - o);
            const size_t stop = f ? (size_t)(f - data) : end;
            out.bytes.insert(out.bytes.end(), data + o, data + stop);
            o = stop;
            if (o >= end) break;
            if (o + 1 < end && data[o + 1] == 0) { out.bytes.push_back(0xFF); o += 2; continue; }      // a stuffed FF
            size_t q = o; while (q < end && data[q] == 0xFF) q++;                                    // fill bytes, then the marker
            if (q < end && data[q] >= 0xD0 && data[q] <= 0xD7) { o = q + 1; at_rst = true; break; }
            data_left = false;                                  // another marker, or FF at the very end: the data ends here
        }
        if (!at_rst && i + 1 < want) {
            if (data_left || o >= end) { if (err.empty()) err = "MJPEG: a restart marker is missing"; }
            data_left = false;
        }
        sg.n_bytes = (uint32_t)(out.bytes.size() - sg.byte_off);
        out.bytes.resize(sg.byte_off + jpeg_entropy_padded(sg.n_bytes), 0);
        sg.first_entry = out.n_entries; sg.entry_cap = jpeg_entropy_capacity(sg.n_bytes, sg.n_mcus * bpm);
        out.n_entries += sg.entry_cap;
        out.segs.push_back(sg);
        if (at_rst && i + 1 == want && err.empty()) err = "MJPEG: more restart markers than the picture has restart intervals (damaged picture)";
    }
    return err;
}

void jpeg_device_tables(const JpegPic &pic, JpegDevHuff out[6]) {
    memset(out, 0, 6 * sizeof(JpegDevHuff));
    for (int c = 0; c < pic.ncomp && c < 3; c++) for (int cls = 0; cls < 2; cls++) {
        const JpegHuff &h = cls ? pic.ac[c] : pic.dc[c]; JpegDevHuff &d = out[3 * cls + c];
        memcpy(d.look, h.look, sizeof d.look); memcpy(d.maxcode, h.maxcode, sizeof d.maxcode);
        memcpy(d.valoff, h.valoff, sizeof d.valoff); memcpy(d.vals, h.vals, sizeof d.vals);
    }
}

bool JpegSplitter::next(size_t &b, size_t &e) {
    const size_t n = in_.size();
    const uint8_t *p = in_.data();
    for (;;) {
        if (state_ == 0) {
            const uint8_t *f = pos_ < n ? (const uint8_t *)memchr(p + pos_, 0xFF, n - pos_) : nullptr;
            if (!f) { pos_ = n; return false; }
            pos_ = (size_t)(f - p);
            if (pos_ + 1 >= n) return false;
            if (p[pos_ + 1] != 0xD8) { pos_++; continue; }
            soi_ = pos_; pos_ += 2; state_ = 1; seen_sos_ = false;
        } else if (state_ == 1) {
            if (pos_ >= n) return false;
            if (p[pos_] != 0xFF) { pos_++; continue; }
            size_t q = pos_;
            while (q < n && p[q] == 0xFF) q++;
            if (q >= n) return false;
            const int m = p[q];
            if (m == 0 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { pos_ = q + 1; continue; }
            if (m == 0xD8) {                                    // a picture begins inside one that never ended
                const bool emit = seen_sos_; b = soi_; e = q - 1;
                soi_ = q - 1; pos_ = q + 1; seen_sos_ = false;
                if (emit) return true;
                continue;
            }
            if (m == 0xD9) { b = soi_; e = q + 1; pos_ = e; state_ = 0; return true; }
            if (q + 2 >= n) return false;
            const size_t len = (size_t)p[q + 1] << 8 | p[q + 2];
            if (len < 2) { pos_ = q + 1; continue; }
            if (q + 1 + len > n) return false;
            pos_ = q + 1 + len;
            if (m == 0xDA) { seen_sos_ = true; state_ = 2; }
        } else {
            const uint8_t *f = pos_ < n ? (const uint8_t *)memchr(p + pos_, 0xFF, n - pos_) : nullptr;
            if (!f) { pos_ = n; return false; }
            pos_ = (size_t)(f - p);
            if (pos_ + 1 >= n) return false;
            const int nx = p[pos_ + 1];
            if (nx == 0 || (nx >= 0xD0 && nx <= 0xD7)) { pos_ += 2; continue; }
            state_ = 1;                                         // a marker (possibly behind fill bytes): RSTn behind fill bytes comes back here
            size_t q = pos_; while (q < n && p[q] == 0xFF) q++;
            if (q >= n) { state_ = 2; return false; }
            if (p[q] >= 0xD0 && p[q] <= 0xD7) { pos_ = q + 1; state_ = 2; }
        }
    }
}

void JpegSplitter::compact() {
    const size_t drop = state_ == 0 ? pos_ : (soi_ > (1u << 16) ? soi_ : 0);
    if (!drop) return;
    in_.erase(in_.begin(), in_.begin() + (long)drop);
    pos_ -= drop; if (state_ != 0) soi_ -= drop; else soi_ = 0;
}

}  // namespace jmamd
