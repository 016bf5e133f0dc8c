// tests/native/mpeg2_vlc_walk.h -- plays k_mpeg2_vlc on the CPU: the prescan (mpeg2_slice_scan) and then mpeg2_vlc_slice, the kernel's own routine,
// once per slice as the kernel's lanes run it.  Every buffer the device would hold is a heap block of exactly the stated size -- tables, picture
// parameters, slice table, slice bytes with their guards, records, entries of exactly the capacity -- so that under AddressSanitizer
// (tools/mpeg2_vlc_asan.cpp) a read or write one element outside any of them is caught.  Shared by tests/native/mpeg2_vlc_check.cpp.
#pragma once
#include "../../jmcodec_amd/csrc/mpeg2_syntax.h"
#include "../../jmcodec_amd/csrc/mpeg2_vlc.h"
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace jmamd {

struct Mpeg2VlcWalk {
    std::string reject;                                            // why the prescan sent the picture to the host path ("" = device path)
    std::vector<Mpeg2Slice> slices;
    std::vector<Mpeg2Mb> mbs; std::vector<uint32_t> entries;       // what the device routine wrote
    std::vector<uint32_t> status; std::vector<uint32_t> used;      // per slice: the routine's result, the entries its span holds
    uint32_t kinds = 0; int damaged = 0, clamped = 0; bool holes = false, dual_prime = false;
    bool bound_ok = true, cap_reached = false, tiled = true;
    bool error() const { return kinds != 0 || holes; }
};

template <class T> static T *m2v_exact_copy(const T *src, size_t n) {      // (malloc: nothing behind the last byte belongs to the block)
    T *p = (T *)malloc(n ? n * sizeof(T) : 1);
    if (n) memcpy(p, src, n * sizeof(T));
    return p;
}

inline void mpeg2_vlc_walk(const Mpeg2Pic &pic, Mpeg2VlcWalk &w) {
    Mpeg2SliceScan sc;
    w = Mpeg2VlcWalk();
    w.reject = mpeg2_slice_scan(pic, sc);
    if (!w.reject.empty()) return;
    w.slices = sc.slices;
    const uint32_t total = (uint32_t)pic.seq.mb_w() * (uint32_t)pic.seq.mb_h();
    const Mpeg2VlcTables *tab = mpeg2_vlc_tables();
    if (!tab || sc.bytes.size() % 4) abort();
    Mpeg2VlcTables *d_tab = m2v_exact_copy(tab, 1);
    const Mpeg2VlcPic vp = mpeg2_vlc_pic(pic);
    Mpeg2VlcPic *d_pic = m2v_exact_copy(&vp, 1);
    Mpeg2Slice *d_slices = m2v_exact_copy(sc.slices.data(), sc.slices.size());
    uint32_t *d_bytes = (uint32_t *)m2v_exact_copy(sc.bytes.data(), sc.bytes.size());
    Mpeg2Mb *d_mbs = (Mpeg2Mb *)aligned_alloc(16, (size_t)total * sizeof(Mpeg2Mb)); memset(d_mbs, 0xEE, (size_t)total * sizeof(Mpeg2Mb));
    uint32_t *d_entries = (uint32_t *)malloc(sc.n_entries ? (size_t)sc.n_entries * 4 : 1); memset(d_entries, 0xEE, (size_t)sc.n_entries * 4);
    // the spans tile the picture, byte offsets are multiples of 4, entry ranges follow each other
    uint32_t at = 0, ent = 0;
    for (const Mpeg2Slice &s : sc.slices) {
        if (s.lo != at || s.hi <= s.lo || s.hi > total || (s.byte_off & 3) || s.first_entry != ent || s.entry_cap != mpeg2_vlc_capacity(s.n_bytes, s.hi - s.lo)) w.tiled = false;
        at = s.hi; ent += s.entry_cap;
    }
    if (at != total || ent != sc.n_entries) w.tiled = false;
    for (size_t i = 0; w.tiled && i < sc.slices.size(); i++) {
        const Mpeg2Slice &s = d_slices[i];
        long long iters = -1;
        const uint32_t st = mpeg2_vlc_slice(*d_pic, d_tab, s, d_bytes, d_mbs, d_entries, &iters);
        if (iters < 0 || iters > mpeg2_vlc_iteration_bound(s.n_bytes, s.hi - s.lo)) w.bound_ok = false;
        // the entries of the span's records lie inside the slice's range, one behind the other
        uint32_t used = 0;
        for (uint32_t a = s.lo; a < s.hi; a++) {
            uint32_t c = 0; for (int k = 0; k < 6; k++) c += d_mbs[a].count[k];
            if (c && (d_mbs[a].first < s.first_entry || d_mbs[a].first + c > s.first_entry + s.entry_cap)) w.bound_ok = false;
            used += c;
        }
        if (used > s.entry_cap) w.bound_ok = false;
        if (!(st & kM2StKindMask) && used == s.entry_cap) w.cap_reached = true;
        w.status.push_back(st); w.used.push_back(used);
        if (st & kM2StKindMask) { w.damaged++; w.kinds |= 1u << (st & kM2StKindMask); }
        w.holes |= (st & kM2StHoles) != 0; w.dual_prime |= (st & kM2StDualPrime) != 0; w.clamped += (int)(st >> kM2StClampedShift);
    }
    w.mbs.assign(d_mbs, d_mbs + total); w.entries.assign(d_entries, d_entries + sc.n_entries);
    free(d_tab); free(d_pic); free(d_slices); free(d_bytes); free(d_mbs); free(d_entries);
}

// Does the walk agree with the host decoder's job list?  Records equal field by field apart from `first`, every block the same entry sequence.
// Returns the number of macroblocks that differ.
inline long mpeg2_vlc_compare(const Mpeg2VlcWalk &w, const Mpeg2Jobs &host) {
    if (w.mbs.size() != host.mbs.size()) return -1;
    long bad = 0;
    for (size_t a = 0; a < w.mbs.size(); a++) {
        Mpeg2Mb x = w.mbs[a], y = host.mbs[a];
        const uint32_t fx = x.first, fy = y.first;
        x.first = y.first = 0;
        bool same = !memcmp(&x, &y, sizeof x);
        uint32_t c = 0; for (int k = 0; k < 6; k++) c += x.count[k];
        if (same && c) same = (size_t)fx + c <= w.entries.size() && (size_t)fy + c <= host.entries.size() && !memcmp(w.entries.data() + fx, host.entries.data() + fy, 4 * (size_t)c);
        bad += !same;
    }
    return bad;
}

}  // namespace jmamd
