// jmcodec_amd/csrc/mpeg2_syntax.h -- MPEG-2 video (codec_type 4, ISO/IEC 13818-2): start-code splitter with picture reassembly, the headers and
// extensions of 6.2, and the slice / macroblock / block VLC decode into the per-picture job list of mpeg2_jobs.h.  What is accepted and what is
// refused: INTEGRATION.md "MPEG-2".  No HIP: the parse pool, tests/native/mpeg2_check.cpp and tools/fuzz_mpeg2.cpp all build it.
#pragma once
#include "mpeg2_jobs.h"
#include "mpeg2_vlc.h"
#include <stddef.h>
#include <string>
#include <vector>

namespace jmamd {

// one entry of a VLC table of Annex B: `len` bits `code`; a, b: what it stands for (table by table: mpeg2_table)
struct Mpeg2Vlc { uint16_t code; uint8_t len; int16_t a, b; };
// the tables as the decoder holds them (tests compare them with the restatement's).  which: 1 B-1 (a = increment; 34 = escape), 2 / 3 / 4 B-2 / B-3 /
// B-4 (a = flags: 1 quant, 2 forward, 4 backward, 8 pattern, 16 intra), 9 B-9 (a = cbp), 10 B-10 (a = |motion_code|, the sign bit follows codes of
// a != 0), 11 B-11 (a = dmvector), 12 / 13 B-12 / B-13 (a = dct_dc_size), 14 / 15 B-14 / B-15 (a = run, b = level, the sign bit follows; a = -1: end of block, -2: escape)
const Mpeg2Vlc *mpeg2_table(int which, int *n);
// scan[alternate_scan][k]: natural position of the k-th coefficient (Figures 7-2, 7-3); the default intra matrix in natural order (6.3.11);
// quantiser_scale of a code (Table 7-6)
extern const uint8_t kMpeg2Scan[2][64], kMpeg2DefaultIntra[64];
int mpeg2_quantiser_scale(int q_scale_type, int code);

// the sequence layer as the pictures that follow it see it
struct Mpeg2Seq {
    bool valid = false;                // a sequence header AND its sequence extension have been read
    int width = 0, height = 0;         // horizontal_size, vertical_size with their extensions
    int aspect = 0, frame_rate_code = 0, fr_ext_n = 0, fr_ext_d = 0;
    int profile_level = 0, progressive_sequence = 0, chroma_format = 1, low_delay = 0;
    bool have_display = false, have_colour = false;          // sequence_display_extension, its colour_description
    int primaries = -1, transfer = -1, matrix = -1, display_w = 0, display_h = 0;
    uint8_t w[2][64] = {{0}};          // intra / non-intra matrix in natural order (quant_matrix_extension overwrites them until the next sequence header)
    int mb_w() const { return (width + 15) / 16; }
    int mb_h() const { return progressive_sequence ? (height + 15) / 16 : 2 * ((height + 31) / 32); }
    void fps(long long *num, long long *den) const;          // frame_rate_value * (n + 1) / (d + 1); 0 / 0 for a forbidden or reserved code
    void sar(int *num, int *den) const;                      // sample aspect ratio from aspect_ratio_information; 0 : 0 when unknown
};

// one picture after its headers: a snapshot of everything the slice decode and the device need
struct Mpeg2Pic {
    Mpeg2Seq seq;
    int temporal_reference = 0, type = 0;                    // picture_coding_type: 1 I, 2 P, 3 B
    int f_code[2][2] = {{15, 15}, {15, 15}};
    int intra_dc_precision = 0, picture_structure = 3, top_field_first = 0, frame_pred_frame_dct = 1, concealment_mv = 0, q_scale_type = 0,
        intra_vlc_format = 0, alternate_scan = 0, repeat_first_field = 0, progressive_frame = 1;
    bool have_ext = false;
    bool field_pictures = false;                             // option mpeg2_field_pictures (Mpeg2Splitter::field_pictures when the picture was cut): field
                                                             // pictures, 16x8 motion compensation and dual prime are decoded, not refused
    bool field() const { return picture_structure == 1 || picture_structure == 2; }
    int mb_h() const { return field() ? seq.mb_h() / 2 : seq.mb_h(); }      // macroblock rows of the picture: a field has half the frame's
    std::vector<uint8_t> data;                               // the picture's slice units, each with its start code 00 00 01 xx in front
};

struct Mpeg2Jobs {
    std::vector<Mpeg2Mb> mbs;          // [mb_w * mb_h], raster order (a field picture: mb_h / 2 rows, Mpeg2Pic::mb_h)
    std::vector<uint32_t> entries;
    int clamped = 0;                   // macroblocks with a vector the host had to clamp
    int n_16x8 = 0, n_dual = 0;        // records with M2_16X8 / M2_DUAL (a picture with one needs Mpeg2PicParams::ext)
};
// Decode the slices of `pic` into records and entries.  Every macroblock gets a record whatever happens: damage (an invalid code, a truncated slice,
// macroblocks no slice covers) is concealed -- zero-vector forward copies in P and B pictures, grey intra blocks in I pictures -- and the reason is
// returned ("" = clean).  *refuse is set when the reason is a feature the decoder refuses (dual prime without pic.field_pictures).
// With pic.field_pictures: the macroblock syntax of field pictures (field_motion_type, no dct_type, a field select with every vector but dual
// prime's), 16x8 and dual prime in P pictures of both structures (in a B picture: damage).  The dual-prime vectors of the opposite parity are derived
// here (7.6.3.6) and every vector, the derived ones included, is clamped so that its block stays inside the reference FIELD.  Concealment in a field
// picture: zero-vector copies of the reference field of the picture's own parity.
std::string mpeg2_decode_picture(const Mpeg2Pic &pic, Mpeg2Jobs &jobs, bool *refuse);

// ---- option mpeg2_device_vlc: the prescan that replaces the slice decode on the host (the decode itself is mpeg2_vlc_slice, mpeg2_vlc.h) ----
// The device form of the Annex B tables, built once per process from mpeg2_table(); nullptr if a table does not fit the two-level scheme.
const Mpeg2VlcTables *mpeg2_vlc_tables();
// the picture's parameters as the device routine reads them
Mpeg2VlcPic mpeg2_vlc_pic(const Mpeg2Pic &pic);
struct Mpeg2SliceScan {
    std::vector<Mpeg2Slice> slices;    // in stream order; their spans tile [0, mb_w * mb_h)
    std::vector<uint8_t> bytes;        // every slice's bytes at its byte_off: padded to a multiple of 4, then kMpeg2SliceGuard zero bytes
    uint32_t n_entries = 0;            // the capacities added up: the size of the device's entry list
};
// One pass over pic.data: per slice the header and the first macroblock_address_increment, nothing more.  "" when the picture can take the device
// path; else why not (a slice header the prescan cannot accept -- quantiser_scale_code 0, a slice outside the picture, an invalid first increment, a
// first address beyond the picture --, first addresses that do not strictly increase, or no slice at all): the host path decodes such a picture.
// A slice without a macroblock (nothing but zero bits behind its header) takes no lane: the host path does nothing with it either.
std::string mpeg2_slice_scan(const Mpeg2Pic &pic, Mpeg2SliceScan &out);

// Incremental front end: feed any chunking of the elementary stream.  Units are cut at start codes, headers are read as they complete, and a picture
// is handed to the sink when the next picture, group, sequence header or sequence end start code arrives, or at flush.
class Mpeg2Splitter {
public:
    template <class Sink> void feed(const uint8_t *buf, size_t len, Sink &&sink) {
        in_.insert(in_.end(), buf, buf + len);
        for (;;) {
            const size_t sc = find_start(scan_);
            if (sc == npos) { scan_ = in_.size() >= 2 ? in_.size() - 2 : 0; if (have_unit_ && scan_ < unit_ + 4) scan_ = unit_ + 3; break; }
            if (have_unit_) { unit(in_.data() + unit_, sc - unit_, sink); }
            have_unit_ = true; unit_ = sc; scan_ = sc + 3;
        }
        if (have_unit_ && unit_ > 0) { in_.erase(in_.begin(), in_.begin() + (long)unit_); scan_ -= unit_; unit_ = 0; }
        else if (!have_unit_ && in_.size() > 2) { in_.erase(in_.begin(), in_.end() - 2); scan_ = 0; }
    }
    // end of stream: the last unit, then the picture in progress
    template <class Sink> void flush(Sink &&sink) {
        if (have_unit_ && in_.size() >= unit_ + 4) unit(in_.data() + unit_, in_.size() - unit_, sink);
        in_.clear(); have_unit_ = false; unit_ = scan_ = 0;
        if (in_pic_) emit(sink);
        expect_seq_ext_ = false;
    }
    // "" or why the stream cannot be decoded; refused(): the reason is a feature the decoder refuses (the handle fails)
    const std::string &error() const { return error_; }
    bool refused() const { return refused_; }
    const Mpeg2Seq &seq() const { return seq_; }
    long long damaged_headers = 0;     // headers that were too short or broke a marker bit (counted, the stream goes on)
    bool field_pictures = false;       // option mpeg2_field_pictures: set before the first feed.  false: field pictures fail the stream, as ever

private:
    static constexpr size_t npos = (size_t)-1;
    size_t find_start(size_t from) const;
    template <class Sink> void unit(const uint8_t *p, size_t n, Sink &&sink) {
        if (refused_ || n < 4) return;                  // (n < 4: a start code right behind a start code prefix, no code byte of its own)
        const int code = p[3];
        // (a picture ends at anything that is not one of its slices, extensions or user data)
        if (in_pic_ && (code == 0x00 || code == 0xB3 || code == 0xB7 || code == 0xB8)) emit(sink);
        header_unit(code, p + 4, n - 4);
        if (code >= 0x01 && code <= 0xAF && in_pic_ && !refused_) pic_.data.insert(pic_.data.end(), p, p + n);
    }
    template <class Sink> void emit(Sink &&sink) {
        in_pic_ = false;
        if (refused_ || !seq_.valid) return;
        pic_.seq = seq_;
        sink(pic_);
        pic_.data.clear();
    }
    void header_unit(int code, const uint8_t *p, size_t n);
    void refuse(const std::string &what) { if (!refused_) { refused_ = true; error_ = what; } }
    std::vector<uint8_t> in_;
    size_t scan_ = 0, unit_ = 0; bool have_unit_ = false;
    Mpeg2Seq seq_; Mpeg2Pic pic_;
    bool in_pic_ = false, expect_seq_ext_ = false, have_seq_hdr_ = false;
    std::string error_; bool refused_ = false;
};

}  // namespace jmamd
