// jmcodec_amd/csrc/out_tables.h -- the job tables of a batch's output stage (engine.cpp: Engine::launch fills them, Engine::run_side launches from them).
//
// A batch packs display frames on two sides of its decode kernels: before them the frames that show earlier pictures, after them the rest (OutSide, jobs.h).
// Each of the four output kernels (k_packout, k_scale_pack, k_rgb_pack, k_deint) has ONE table of 4 * kMaxBatch jobs: the before side starts at entry 0, the
// after side at 2 * kMaxBatch; entries are in picture order and, within a picture, in the order the decoder queued them.  The launch grids are maxima over
// BOTH sides (one figure per kernel and batch).  A deinterlaced frame of a scaled / RGB handle passes through a surface in the batch's scratch: k_deint
// writes it, the ScaleJob / RgbJob at DeintReq::index of the same picture and side reads it; surfaces are handed out in the order of the add() calls, each
// rounded up to 256 bytes.  A field-rate pair (DeintReq::pair) is ONE entry of k_deint's table with two destinations and, for a scaled / RGB handle, two
// scratch surfaces (first field first) read by the jobs at DeintReq::index and index2; it counts as two frames.  pairs[side] says whether a side holds one
// (the engine then launches the table through k_deint2), temporal[side] whether it holds a job that reads a previous frame (DeintJob::prev: k_deint3).
// Host code, header-only, no HIP: the tables' memory is the caller's.  tests/test_out_tables.py checks the layout against a restatement of these rules.
#pragma once
#include "jobs.h"
#include <algorithm>

namespace jmamd {

constexpr int kMaxBatch = 64;                       // pictures of one launch
constexpr int kOutSideCap = 2 * kMaxBatch;          // table entries of one side: Engine::form keeps a batch's frames per side within it
enum : int { kBefore = 0, kAfter = 1 };             // the sides

// the grid a job needs, defined beside its kernel (out_kernels.hip)
int scale_tiles(int tw, int th);
int rgb_tiles(int tw, int th);
int deint_items(int w, int h);

template <class J> struct JobTable {
    J *host = nullptr, *dev = nullptr;              // 2 * kOutSideCap entries each (the engine: pinned host memory and its copy on the device)
    int n[2] = {0, 0};                              // entries in use per side
    J *h(int side) const { return host + side * kOutSideCap; }
    const J *d(int side) const { return dev + side * kOutSideCap; }
};

struct OutTables {
    JobTable<PackJob> plain; JobTable<ScaleJob> scale; JobTable<RgbJob> rgb; JobTable<DeintJob> deint;
    template <class F> void each(F &&f) { f(plain); f(scale); f(rgb); f(deint); }
    // grids: k_packout's frame size (over the pictures with a plain job), launch_scale_pack's tiles, launch_rgb_pack's (identity / resampled jobs / jobs with interpolated chroma), launch_deint's
    int max_w = 0, max_h = 0, s_tiles = 0, r_tiles[3] = {0, 0, 0}, d_items = 0, pairs[2] = {0, 0}, temporal[2] = {0, 0};
    int n_chroma[2] = {0, 0};                       // per side: RGB jobs with interpolated chroma (r_tiles[2] is their grid; k_rgb_pack444)
    // profiling sums: frames and their algorithmic bytes -- of every output kernel together, of k_rgb_pack alone, of k_deint alone
    long long alg_pack = 0, alg_rgb = 0, alg_deint = 0, alg_rgb444 = 0; int n_frames = 0, n_rgb = 0, n_deint = 0;
    uint8_t *scratch = nullptr; size_t scratch_used = 0;

    static size_t scratch_bytes(const DeintJob &j) { return ((size_t)j.dst_pitch * j.height * 3 / 2 + 255) & ~(size_t)255; }
    // scratch the frames of one side of a picture need (the caller adds up its batch and grows the allocation before reset())
    static size_t bytes_needed(const OutSide &o) { size_t n = 0; for (auto &r : o.deint) if (r.feeds) n += scratch_bytes(r.job) * (r.pair() ? 2 : 1); return n; }
    bool any(int side) const { return plain.n[side] || scale.n[side] || rgb.n[side] || deint.n[side]; }

    void reset(uint8_t *scratch_base) {
        each([](auto &t) { t.n[0] = t.n[1] = 0; });
        max_w = max_h = s_tiles = r_tiles[0] = r_tiles[1] = r_tiles[2] = d_items = pairs[0] = pairs[1] = temporal[0] = temporal[1] = n_chroma[0] = n_chroma[1] = 0;
        alg_pack = alg_rgb = alg_deint = alg_rgb444 = 0; n_frames = n_rgb = n_deint = 0;
        scratch = scratch_base; scratch_used = 0;
    }
    // The frames of one side of one picture; pictures in batch order, a picture's before side first.  disp_w / disp_h: the picture's display size;
    // pack_bytes / deint_bytes: algorithmic bytes of one of its frames in a pack kernel / in k_deint (a pair: 3 / 2 of it).  false: a frame needed scratch and there is none
    // (scratch_base was null) -- its k_deint job is left out and its ScaleJob / RgbJob reads the picture's surface instead; the caller fails the handle.
    bool add(const OutSide &o, int side, int disp_w, int disp_h, long long pack_bytes, long long deint_bytes) {
        ScaleJob *s0 = scale.h(side) + scale.n[side]; RgbJob *r0 = rgb.h(side) + rgb.n[side];       // this picture's first entries
        for (auto &j : o.plain) plain.h(side)[plain.n[side]++] = j;
        if (!o.plain.empty()) { max_w = std::max(max_w, disp_w); max_h = std::max(max_h, disp_h); }
        for (auto &j : o.scale) { scale.h(side)[scale.n[side]++] = j; s_tiles = std::max(s_tiles, scale_tiles(j.tw, j.th)); }
        for (auto &j : o.rgb) { rgb.h(side)[rgb.n[side]++] = j; int &t = r_tiles[j.chroma ? 2 : j.identity ? 0 : 1]; t = std::max(t, rgb_tiles(j.s.tw, j.s.th));
            if (j.chroma) { n_chroma[side]++; alg_rgb444 += pack_bytes; } }
        bool ok = true;
        for (auto &r : o.deint) {
            DeintJob j = r.job;
            const bool pair = r.pair();
            if (r.feeds) {
                const uint8_t *&src = r.feeds == 1 ? s0[r.index].src : r0[r.index].s.src;
                const uint8_t *&src2 = r.feeds == 1 ? s0[pair ? r.index2 : r.index].src : r0[pair ? r.index2 : r.index].s.src;
                if (!scratch) { src = src2 = j.src; ok = false; continue; }
                j.dst = scratch + scratch_used; src = j.dst; scratch_used += scratch_bytes(j);
                if (pair) { j.dst2 = scratch + scratch_used; src2 = j.dst2; scratch_used += scratch_bytes(j); }
            }
            deint.h(side)[deint.n[side]++] = j;
            d_items = std::max(d_items, deint_items(j.width, j.height));        // (a pair has no more items than a frame: the grid covers it)
            // (a pair reads the surface once and writes two frames: 3 S against a frame's 2 S)
            // (a job with a previous frame reads that surface too: 3 S and 4 S; temporal[side]: the side goes through k_deint3)
            if (j.prev) temporal[side]++;
            if (pair) { pairs[side]++; alg_deint += deint_bytes * (j.prev ? 4 : 3) / 2; n_deint += 2; }
            else { alg_deint += deint_bytes * (j.prev ? 3 : 2) / 2; n_deint++; }
        }
        const int f = (int)o.frames(), nr = (int)o.rgb.size();
        alg_pack += pack_bytes * f; n_frames += f; alg_rgb += pack_bytes * nr; n_rgb += nr;
        return ok;
    }
};

}  // namespace jmamd
