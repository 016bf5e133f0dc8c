// jmcodec_amd/csrc/jpeg_syntax.h -- MJPEG (codec_type 2): marker parser, canonical Huffman decode and the per-picture sparse job list.
// ITU-T T.81 baseline / extended sequential Huffman, 8 bits, one interleaved scan; what is accepted and what is refused: INTEGRATION.md "MJPEG".
// No HIP: the parse pool, tests/native/jpeg_check.cpp and tools/fuzz_jpeg.cpp all build it.
#pragma once
#include "jpeg_entropy.h"
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>

namespace jmamd {

struct JpegHuff {
    bool set = false;
    uint8_t bits[17] = {0}, vals[256] = {0};
    // lookup by the next 9 bits: length << 8 | symbol (0: longer than 9 bits or invalid); codes of length l: maxcode[l] (-1: none), valoff[l]
    uint16_t look[512] = {0};
    int32_t maxcode[18] = {0}, valoff[17] = {0};
    bool build();                  // false: the lengths do not describe a prefix code, or more than 256 symbols
};

// what persists from picture to picture within a handle (T.81 B.2.4: tables stay defined until they are redefined)
struct JpegTables {
    uint8_t q[4][64] = {{0}}; bool q_set[4] = {false, false, false, false};      // zig-zag order
    JpegHuff dc[4], ac[4];
    int restart_interval = 0;
};

// one picture after its headers: everything the entropy decode and the device need (a snapshot: the handle's tables may change for the next picture)
struct JpegPic {
    int width = 0, height = 0, ncomp = 0, sampling = 0;       // sampling: 0x22 / 0x21 / 0x11 / 0x10 (grey)
    int mcu_w = 0, mcu_h = 0, mcus_x = 0, mcus_y = 0;         // MCU size in luma samples, MCUs per row / rows
    int y_bw = 0, y_bh = 0, c_bw = 0, c_bh = 0;               // blocks of the luma plane / one chroma plane
    int restart_interval = 0;
    uint8_t q[3][64] = {{0}};
    JpegHuff dc[3], ac[3];                                    // per component
    size_t scan_off = 0, scan_end = 0;                        // entropy-coded data: [scan_off, scan_end) of the picture's bytes
    bool used_default_huff = false;                           // no DHT seen so far in the handle: the tables of T.81 Annex K.3
    int disp_w() const { return (width + 1) & ~1; }
    int disp_h() const { return (height + 1) & ~1; }
    int n_blocks() const { return y_bw * y_bh + (ncomp == 3 ? 2 * c_bw * c_bh : 0); }
};

// T.81 Annex K.3 "typical" tables (Tables K.3 - K.6), used by pictures of a stream that never sent a DHT (AVI-style MJPEG)
extern const uint8_t kJpegStdDcLumaBits[16], kJpegStdDcLumaVals[12], kJpegStdDcChromaBits[16], kJpegStdDcChromaVals[12];
extern const uint8_t kJpegStdAcLumaBits[16], kJpegStdAcLumaVals[162], kJpegStdAcChromaBits[16], kJpegStdAcChromaVals[162];

// Walk the segments of one picture p[0 .. n) (it starts at SOI; n ends behind EOI, or where the data ends).  Updates `tab` (DQT, DHT, DRI).
// Returns "" and fills pic, or the reason the picture cannot be decoded; *refuse is set when the reason is a feature the decoder refuses
// (the handle then fails: INTEGRATION.md) and left alone when the picture is merely damaged.
std::string jpeg_parse_picture(const uint8_t *p, size_t n, JpegTables &tab, JpegPic &pic, bool *refuse);

struct JpegJobs {
    std::vector<uint32_t> first;       // per block (plane raster order: Y, Cb, Cr): index of its first entry
    std::vector<uint8_t> count;        // ... and how many it has (0 .. 64)
    std::vector<uint32_t> entries;     // zig-zag position | (uint16_t)level << 16, non-zero levels only
};
// Entropy-decode the scan of `pic` (data = the picture's bytes, as given to jpeg_parse_picture).  Every block gets a record whatever happens: after
// damage (truncation, an invalid code, a missing restart marker) decoding stops, the remaining blocks are empty and the reason is returned.
std::string jpeg_decode_scan(const JpegPic &pic, const uint8_t *data, size_t n, JpegJobs &jobs);

// Option jpeg_device_entropy: what the device needs to entropy-decode the scan itself (jpeg_entropy.h has the layout and the routine).
struct JpegSegments {
    std::vector<JpegSegment> segs;     // one per restart interval (one for the whole scan without DRI); every MCU belongs to exactly one
    std::vector<uint8_t> bytes;        // the segments' clean bytes: unstuffed, each padded to 4 bytes + kJpegSegGuard zeros
    uint32_t n_entries = 0;            // sum of the segments' entry capacities
};
// One linear pass over [scan_off, scan_end) of `data`.  Fill bytes and RSTn markers (any index) are removed.  Fewer markers than the picture's
// intervals need: the MCUs not covered get empty segments (length 0) and the reason is returned; more: the surplus is dropped and the reason is
// returned.  The picture is decodable either way.
std::string jpeg_segment_scan(const JpegPic &pic, const uint8_t *data, size_t n, JpegSegments &out);
// the device form of the picture's tables: DC of components 0..2, then AC (components a grey picture lacks: zeros)
void jpeg_device_tables(const JpegPic &pic, JpegDevHuff out[6]);
inline JpegScanGeom jpeg_scan_geom(const JpegPic &pic) {
    return JpegScanGeom{pic.ncomp, pic.mcu_w / 8, pic.mcu_h / 8, pic.mcus_x, pic.y_bw, pic.y_bh, pic.c_bw, pic.c_bh};
}
// segments a picture's scan consists of by its headers
inline long long jpeg_expected_segments(const JpegPic &pic) {
    const long long mcus = (long long)pic.mcus_x * pic.mcus_y;
    return pic.restart_interval > 0 ? (mcus + pic.restart_interval - 1) / pic.restart_interval : 1;
}

// Incremental picture splitter: feed any chunking of a byte stream of concatenated pictures; complete pictures come out whole.
class JpegSplitter {
public:
    // appends data; for every picture completed calls sink(bytes, length, false)
    template <class Sink> void feed(const uint8_t *buf, size_t len, Sink &&sink) {
        in_.insert(in_.end(), buf, buf + len);
        size_t b, e;
        while (next(b, e)) sink(in_.data() + b, e - b, false);
        compact();
    }
    // end of stream: a picture that was begun and whose scan has started is handed to sink(bytes, length, true); returns whether bytes were dropped
    template <class Sink> bool flush(Sink &&sink) {
        bool dropped = false;
        if (state_ != 0) { if (seen_sos_) sink(in_.data() + soi_, in_.size() - soi_, true); else dropped = in_.size() > soi_ + 2; }
        in_.clear(); pos_ = soi_ = 0; state_ = 0; seen_sos_ = false;
        return dropped;
    }
private:
    bool next(size_t &b, size_t &e);
    void compact();
    std::vector<uint8_t> in_;
    size_t pos_ = 0, soi_ = 0;
    int state_ = 0;                    // 0 looking for SOI, 1 at a marker, 2 inside entropy-coded data
    bool seen_sos_ = false;
};

}  // namespace jmamd
