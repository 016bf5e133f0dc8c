// jmcodec_amd/csrc/vp8_syntax.h -- VP8 (codec_type 5): IVF / frame-per-call input, the frame header, the bool decoder, the per-macroblock modes of the
// first partition and the token decode of the token partitions of a key frame and, with option vp8_inter, of an inter frame (RFC 6386), into the job
// list of vp8_jobs.h.  An inter frame's parse depends on what the frames before it left behind (Vp8State): a stream's frames are parsed in order.
// What is accepted and what is refused: INTEGRATION.md "VP8".  No HIP: the parse pool, tests/native/vp8_check.cpp and tools/fuzz_vp8.cpp build it.
#pragma once
#include "vp8_jobs.h"
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

namespace jmamd {

// the tables of RFC 6386, typed in from its sections 14.1, 13.4, 13.5, 11.2 - 11.5 and 13.2 (tests/test_vp8_host.py compares them with the
// restatement's own, through tests/native/vp8_check.cpp)
extern const uint8_t kVp8DcQ[128];
extern const uint16_t kVp8AcQ[128];
extern const uint8_t kVp8CoefProbs[4][8][3][11];          // default coefficient probabilities
extern const uint8_t kVp8CoefUpdateProbs[4][8][3][11];
extern const uint8_t kVp8KfYmodeProb[4], kVp8KfUvModeProb[3];
extern const uint8_t kVp8KfBmodeProbs[10][10][9];         // [above][left]
extern const int8_t kVp8KfYmodeTree[8], kVp8UvModeTree[6], kVp8BmodeTree[18], kVp8SegmentTree[6], kVp8CoefTree[22];
extern const uint8_t kVp8CoefBands[16], kVp8Zigzag[16];
extern const uint8_t kVp8CatProbs[6][12];                 // zero-terminated
extern const uint8_t kVp8CatBase[6];
// inter frames (sections 16.2, 16.3, 17.2 and the decoder printed in the RFC); tests/test_vp8_inter_host.py compares them with the restatement's own
extern const uint8_t kVp8YmodeProb[4], kVp8UvModeProb[3], kVp8BmodeProb[9];      // the defaults of frames that are no key frames
extern const int8_t kVp8YmodeTree[8], kVp8MvRefTree[8], kVp8SubMvRefTree[6], kVp8SplitTree[6], kVp8SmallMvTree[14];
extern const uint8_t kVp8ModeContexts[6][4], kVp8SubMvRefProbs[5][3], kVp8SplitProbs[3];
extern const uint8_t kVp8MvDefaultProbs[2][19], kVp8MvUpdateProbs[2][19];        // [0] rows, [1] columns: is_short, sign, 7 short-tree, 10 long bits
extern const uint8_t kVp8Splits[4][16];                                          // the partition each luma block belongs to: 16x8, 8x16, 8x8, 4x4

constexpr int kVp8MaxDim = 8192;                          // (the MJPEG path's limit)

// RFC 6386 7.3.  Bounds-safe: past the end of its bytes the decoder reads zeros, and counts them.
struct Vp8Bool {
    const uint8_t *p = nullptr, *end = nullptr;
    uint32_t value = 0, range = 255;
    int bit_count = 0;
    long long past = 0;
    void init(const uint8_t *b, size_t n) { p = b; end = b + n; past = 0; range = 255; bit_count = 0; value = next() << 8; value |= next(); }
    uint32_t next() { if (p < end) return *p++; past++; return 0; }
    int read(int prob) {
        const uint32_t split = 1 + (((range - 1) * (uint32_t)prob) >> 8), big = split << 8;
        int bit;
        if (value >= big) { bit = 1; range -= split; value -= big; } else { bit = 0; range = split; }
        while (range < 128) { value <<= 1; range <<= 1; if (++bit_count == 8) { bit_count = 0; value |= next(); } }
        return bit;
    }
    int literal(int n) { int v = 0; while (n--) v = v << 1 | read(128); return v; }
    int flagged(int n) { if (!read(128)) return 0; const int v = literal(n); return read(128) ? -v : v; }
    int tree(const int8_t *t, const uint8_t *probs, int start = 0) { int i = start; do i = t[i + read(probs[i >> 1])]; while (i > 0); return -i; }
};

// what the first ten bytes of a frame say (the caller thread reads them: size changes, refusals)
struct Vp8FrameTag {
    bool key = false; int version = 0, show = 0; uint32_t part1 = 0;
    int width = 0, height = 0, hscale = 0, vscale = 0;
};
// "" or why the frame is refused (a handle fails on it).  first: no key frame has been decoded yet.  inter_ok (option vp8_inter): a frame that is
// no key frame is accepted behind a key frame; its three bytes carry no size -- width and height stay what the caller put into tag
std::string vp8_read_tag(const uint8_t *p, size_t n, bool first, Vp8FrameTag &tag, bool inter_ok = false);

// What a stream's frames hand to the next one (RFC 6386 9.3, 9.6, 9.7, 9.10, 9.11): the probabilities, the segment map and data, the loop-filter deltas,
// the sign biases, and per macroblock what the near-vector search of the NEXT ROW reads.  A key frame resets all of it.
struct Vp8Entropy { uint8_t coef[4][8][3][11], mv[2][19], ymode[4], uvmode[3]; };
struct Vp8State {
    Vp8Entropy e;
    int seg_abs = 0, seg_q[4] = {0, 0, 0, 0}, seg_lf[4] = {0, 0, 0, 0};
    int ref_delta[4] = {0, 0, 0, 0}, mode_delta[4] = {0, 0, 0, 0};
    int sign_bias[4] = {0, 0, 0, 0};       // indexed by reference: 2 golden, 3 altref (0 and 1 stay 0)
    int mb_w = 0, mb_h = 0;
    std::vector<uint8_t> seg_map;          // [mb_w * mb_h]
    void reset_key(int w, int h);
};

// one decoded frame: header fields, what the stream exercised, the job list
struct Vp8Pic {
    Vp8FrameTag tag;
    int mb_w = 0, mb_h = 0;
    int color_space = 0, clamping = 0;
    int seg_on = 0, update_map = 0, seg_abs = 0;
    int filter_type = 0, level = 0, sharpness = 0, delta_on = 0;
    int n_parts = 1, refresh_entropy = 0, no_coeff_skip = 0, prob_updates = 0;
    int16_t dq[4][6] = {{0}};
    bool damaged = false;              // a partition overruns the frame, or a bool decoder read more than two bytes past its end
    bool filtered = false;             // some macroblock has a non-zero filter level
    int bpred_mbs = 0, skipped_mbs = 0, segments_used = 0;     // segments_used: bit mask
    std::vector<Vp8Mb> mbs;
    std::vector<uint32_t> entries;
    // inter frames (all zero / empty on a key frame)
    int refresh_golden = 0, refresh_alt = 0, copy_to_golden = 0, copy_to_alt = 0, refresh_last = 1;
    int prob_intra = 0, prob_last = 0, prob_gf = 0, mode_prob_updates = 0, mv_prob_updates = 0;
    int inter_mbs = 0, golden_mbs = 0, alt_mbs = 0, split_mbs = 0, intra_mbs = 0;
    std::vector<Vp8SplitMv> split;     // one per SPLITMV macroblock, in raster order of those macroblocks
};
// Decode the frame p[0 .. n) (vp8_read_tag accepted it).  Every macroblock gets a record whatever the bytes hold.  st: the stream's state, read and
// left for the next frame; nullptr: key frames only, each from the defaults (the frames of a handle without option vp8_inter).
void vp8_decode_frame(const uint8_t *p, size_t n, Vp8Pic &pic, Vp8State *st = nullptr);
// every field the device indexes with: modes, segment, level, first / count against the entry list, block numbers; "" or what is wrong
std::string vp8_validate_jobs(const Vp8Pic &pic);

// Input (INTEGRATION.md "VP8"): a stream that begins with "DKIF" is an IVF byte stream in any chunking -- a 32-byte header, then per frame a 12-byte
// header (size, pts) and the payload; any other stream is one whole frame per feed() call.  While fewer than four bytes have arrived and they are a
// prefix of "DKIF" the decision waits for the next call.
class Vp8Splitter {
public:
    // sink(frame, length, truncated); a frame of length 0 is reported too (the decoder counts and skips it)
    template <class Sink> void feed(const uint8_t *buf, size_t len, Sink &&sink) {
        if (mode_ == 2) { sink(buf, len, false); return; }
        in_.insert(in_.end(), buf, buf + len);
        if (mode_ == 0) {
            const size_t k = in_.size() < 4 ? in_.size() : 4;
            if (memcmp_dkif(k)) { if (in_.size() < 4) return; mode_ = 1; }
            else { mode_ = 2; std::vector<uint8_t> f; f.swap(in_); sink(f.data(), f.size(), false); return; }
        }
        size_t o = pos_;
        for (;;) {
            if (!header_done_) { if (in_.size() - o < 32) break; o += 32; header_done_ = true; }
            if (in_.size() - o < 12) break;
            const size_t n = (size_t)in_[o] | (size_t)in_[o + 1] << 8 | (size_t)in_[o + 2] << 16 | (size_t)in_[o + 3] << 24;
            if (in_.size() - o - 12 < n) break;
            sink(in_.data() + o + 12, n, false);
            o += 12 + n;
        }
        in_.erase(in_.begin(), in_.begin() + (ptrdiff_t)o); pos_ = 0;
    }
    // end of stream: a frame cut off by the end is handed out as far as it goes (truncated); returns whether other bytes were dropped
    template <class Sink> bool flush(Sink &&sink) {
        bool dropped = false;
        if (mode_ == 1 && header_done_ && in_.size() >= 12) sink(in_.data() + 12, in_.size() - 12, true);
        else dropped = !in_.empty();
        in_.clear(); pos_ = 0; mode_ = 0; header_done_ = false;
        return dropped;
    }
private:
    bool memcmp_dkif(size_t k) const { static const char m[4] = {'D', 'K', 'I', 'F'}; for (size_t i = 0; i < k; i++) if (in_[i] != (uint8_t)m[i]) return false; return true; }
    std::vector<uint8_t> in_;
    size_t pos_ = 0;
    int mode_ = 0;                     // 0 undecided, 1 IVF, 2 one frame per call
    bool header_done_ = false;
};

}  // namespace jmamd
