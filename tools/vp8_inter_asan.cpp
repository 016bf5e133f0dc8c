// tools/vp8_inter_asan.cpp -- option vp8_inter on the CPU under AddressSanitizer / UBSan (host sanitizers; `make -C tools vp8_inter_asan`): the lane routines
// of vp8_recon.h that k_vp8_inter, k_vp8_recon and k_vp8_filter run, over heap surfaces and reference surfaces of EXACTLY the device's extent
// (16 mb_w x 16 mb_h luma samples + chroma, pitch = 16 mb_w).  A read outside a reference window's surface, a store outside the picture, the job list,
// the split list or a work area is caught.  A stand-alone program with its own main; nothing here touches a device.
//   vp8_inter_asan <seed> <trials>                 random job lists at the sizes of the GPU tests: every macroblock of every border with vectors
//                                                  that point far beyond each edge (any 16-bit value), whole and split, six-tap and bilinear; valid
//                                                  lists (what vp8_validate_jobs accepts) and damaged ones (the routines clamp what they index with)
//   vp8_inter_asan <seed> <trials> <stream.ivf>    the sibling of fuzz_vp8 for inter streams: trial 0 feeds the stream as it is, the others flip,
//                                                  insert, delete and truncate bytes; frames are parsed with the stream's state and predicted from
//                                                  the references the headers name.  A job list the parser wrote must always validate
#include "../jmcodec_amd/csrc/vp8_syntax.h"
#include "../jmcodec_amd/csrc/vp8_recon.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

using namespace jmamd;

namespace {
struct Surf { std::unique_ptr<uint8_t[]> p; int W = 0, H = 0; size_t bytes() const { return (size_t)W * H * 3 / 2; } };
std::shared_ptr<Surf> make_surf(int W, int H, std::mt19937 *rng) {
    auto s = std::make_shared<Surf>();
    s->W = W; s->H = H; s->p.reset(new uint8_t[s->bytes()]);
    for (size_t i = 0; i < s->bytes(); i++) s->p[i] = rng ? (uint8_t)(*rng)() : 128;
    return s;
}

int random_lists(std::mt19937 &rng, int trials) {
    static const int sizes[][2] = {{16, 16}, {48, 32}, {53, 37}, {272, 16}, {16, 272}, {80, 272}};
    static const int16_t edge[] = {0, 2, -2, 6, 126, -130, 1022, -1026, 4094, -4098, 32766, -32768, 2046, -2046};
    long pictures = 0, invalid = 0; unsigned long long sum = 0;
    for (int t = 0; t < trials; t++) for (auto &sz : sizes) {
        const int mb_w = (sz[0] + 15) / 16, mb_h = (sz[1] + 15) / 16, n = mb_w * mb_h;
        const bool damage = t % 2 == 1;
        std::unique_ptr<Vp8Mb[]> mbs(new Vp8Mb[n]);
        std::vector<uint32_t> ent; std::vector<Vp8SplitMv> split;
        int n_intra = 0;
        auto vec = [&]() { return (int16_t)(rng() % 3 == 0 ? edge[rng() % (sizeof edge / sizeof edge[0])] : (int)(rng() % 65536) - 32768); };
        for (int i = 0; i < n; i++) {
            Vp8Mb &m = mbs[i]; memset(&m, 0, sizeof m);
            const bool inter = rng() % 5 != 0;
            m.uvmode = (uint8_t)(rng() % 4); m.segment = (uint8_t)(rng() % 4); m.level = (uint8_t)(rng() % 64);
            if (inter) {
                Vp8InterInfo ii; memset(&ii, 0, sizeof ii);
                ii.ref = (uint8_t)(1 + rng() % 3); ii.mvx = vec(); ii.mvy = vec(); ii.cmvx = vec(); ii.cmvy = vec();
                if (rng() % 3 == 0) {
                    ii.split = (uint8_t)(1 + rng() % 4); ii.split_idx = (uint32_t)split.size();
                    Vp8SplitMv sv;
                    for (auto &v : sv.y) { v[0] = vec(); v[1] = vec(); }
                    for (auto &v : sv.c) { v[0] = vec(); v[1] = vec(); }
                    split.push_back(sv);
                }
                m.flags = VP8_MB_INTER; m.mvmode = ii.split ? VP8_MV_SPLIT : (uint8_t)(1 + rng() % 4); m.ymode = ii.split ? VP8_B_PRED : VP8_DC_PRED; m.uvmode = 0;
                memcpy(m.bmodes, &ii, sizeof ii);
            } else {
                m.ymode = (uint8_t)(rng() % 5);
                for (auto &b : m.bmodes) b = (uint8_t)(rng() % 10);
                n_intra++;
            }
            m.first = (uint32_t)ent.size();
            const int cnt = (int)(rng() % 3 == 0 ? 0 : rng() % 60);
            for (int e = 0; e < cnt; e++) {
                const int blk = (int)(rng() % (m.ymode == VP8_B_PRED ? 24 : 25)), lv = (int)(rng() % 4200) - 2100;
                ent.push_back((uint32_t)(rng() % 16) | (uint32_t)blk << 4 | (uint32_t)(uint16_t)(int16_t)lv << 16);
                m.nz |= 1u << blk;
            }
            m.count = (uint16_t)cnt;
            if (cnt || m.ymode == VP8_B_PRED) m.flags |= VP8_MB_INNER;
            if (damage && rng() % 3 == 0) switch (rng() % 7) {
                case 0: m.ymode = (uint8_t)rng(); break;
                case 1: m.uvmode = (uint8_t)rng(); m.segment = (uint8_t)rng(); break;
                case 2: m.level = (uint8_t)rng(); m.flags = (uint8_t)rng(); break;
                case 3: m.first = (uint32_t)rng(); break;
                case 4: m.count = (uint16_t)rng(); m.nz = (uint32_t)rng(); break;
                case 5: m.mvmode = (uint8_t)rng(); m.bmodes[0] = (uint8_t)rng(); m.bmodes[1] = (uint8_t)rng(); { uint32_t v = (uint32_t)rng(); memcpy(m.bmodes + 12, &v, 4); } break;
                default: for (auto &b : m.bmodes) b = (uint8_t)rng(); break;
            }
        }
        if (damage) for (auto &e : ent) if (rng() % 8 == 0) e = (uint32_t)rng();
        std::unique_ptr<uint32_t[]> entries(new uint32_t[ent.size() ? ent.size() : 1]);
        if (!ent.empty()) memcpy(entries.get(), ent.data(), ent.size() * 4);
        std::unique_ptr<Vp8SplitMv[]> sp(new Vp8SplitMv[split.size() ? split.size() : 1]);
        if (!split.empty()) memcpy(sp.get(), split.data(), split.size() * sizeof(Vp8SplitMv));
        const int W = mb_w * 16, H = mb_h * 16;
        auto cur = make_surf(W, H, nullptr);
        std::shared_ptr<Surf> refs[3] = {make_surf(W, H, &rng), make_surf(W, H, &rng), make_surf(W, H, &rng)};
        Vp8PicParams pp = {};
        pp.surf = cur->p.get(); pp.pitch = W; pp.chroma_offset = W * H; pp.mb_w = mb_w; pp.mb_h = mb_h;
        pp.n_entries = (int)ent.size(); pp.filter_type = (int)(rng() % 2); pp.sharpness = (int)(rng() % 8); pp.filtered = 1;
        pp.mbs = mbs.get(); pp.entries = entries.get();
        pp.inter = 1; pp.interp = (int)(rng() % 2); pp.n_intra = n_intra; pp.n_split = (int)split.size(); pp.split = sp.get();
        for (int k = 0; k < 3; k++) pp.ref[k] = damage && rng() % 7 == 0 ? nullptr : refs[k]->p.get();
        for (auto &s : pp.dq) for (auto &q : s) q = (int16_t)(4 + rng() % 437);
        Vp8Pic pic; pic.tag.key = false; pic.mb_w = mb_w; pic.mb_h = mb_h; pic.mbs.assign(mbs.get(), mbs.get() + n); pic.entries = ent; pic.split = split;
        const std::string v = vp8_validate_jobs(pic);
        if (!damage && !v.empty()) { fprintf(stderr, "a valid list was not accepted: %s\n", v.c_str()); return 1; }
        if (damage && !v.empty()) invalid++;
        vp8_inter_host(pp);
        vp8_reconstruct_host(pp);
        vp8_filter_host(pp);
        for (size_t i = 0; i < cur->bytes(); i += 97) sum += cur->p[i];
        pictures++;
    }
    printf("ok: %d trials, %ld pictures predicted, reconstructed and filtered, %ld damaged lists the validation refuses, checksum %llu\n", trials, pictures, invalid, sum);
    return 0;
}

int fuzz_stream(std::mt19937 &rng, int trials, const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return 2; }
    std::vector<uint8_t> src; { uint8_t buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) src.insert(src.end(), buf, buf + k); }
    fclose(f);
    long pictures = 0, inter = 0, damaged = 0, refused = 0, empty = 0; int bad = 0;
    for (int t = 0; t < trials; t++) {
        std::vector<uint8_t> d = src;
        if (t > 0 && !d.empty()) {
            const int n_mut = 1 + (int)(rng() % 8);
            for (int m = 0; m < n_mut && !d.empty(); m++) {
                const size_t at = rng() % d.size();
                switch (rng() % 5) {
                case 0: d[at] ^= (uint8_t)(1u << (rng() % 8)); break;
                case 1: d[at] = (uint8_t)rng(); break;
                case 2: d.insert(d.begin() + (long)at, (uint8_t)(rng() % 2 ? 0x00 : rng())); break;
                case 3: d.erase(d.begin() + (long)at); break;
                default: if (rng() % 4 == 0) d.resize(at); break;
                }
            }
        }
        Vp8Splitter sp; Vp8State state; std::shared_ptr<Surf> ref[3]; long keys = 0; bool stop = false; int width = 0, height = 0;
        auto sink = [&](const uint8_t *p, size_t n, bool truncated) {
            if (stop) return;
            if (n == 0) { empty++; return; }
            std::unique_ptr<uint8_t[]> frame(new uint8_t[n]);            // exactly the frame: the bool decoders may not read beyond it
            memcpy(frame.get(), p, n);
            Vp8Pic pic;
            if (!vp8_read_tag(frame.get(), n, keys == 0, pic.tag, true).empty()) { refused++; stop = true; return; }
            if (pic.tag.key) { width = pic.tag.width; height = pic.tag.height; } else { pic.tag.width = width; pic.tag.height = height; }
            if (width > 1024 || height > 1024) { stop = true; return; }  // (a mutated size field: keep the trial short)
            vp8_decode_frame(frame.get(), n, pic, &state);
            const std::string v = vp8_validate_jobs(pic);
            if (!v.empty()) { fprintf(stderr, "trial %d: the parser's own job list does not validate: %s\n", t, v.c_str()); bad = 1; stop = true; return; }
            if (pic.tag.key) keys++; else inter++;
            if (pic.damaged || truncated) damaged++;
            const int W = pic.mb_w * 16, H = pic.mb_h * 16;
            auto cur = make_surf(W, H, nullptr);
            std::unique_ptr<uint32_t[]> entries(new uint32_t[pic.entries.size() ? pic.entries.size() : 1]);
            if (!pic.entries.empty()) memcpy(entries.get(), pic.entries.data(), pic.entries.size() * 4);
            std::unique_ptr<Vp8SplitMv[]> spl(new Vp8SplitMv[pic.split.size() ? pic.split.size() : 1]);
            if (!pic.split.empty()) memcpy(spl.get(), pic.split.data(), pic.split.size() * sizeof(Vp8SplitMv));
            Vp8PicParams pp = {};
            pp.surf = cur->p.get(); pp.pitch = W; pp.chroma_offset = W * H; pp.mb_w = pic.mb_w; pp.mb_h = pic.mb_h;
            pp.n_entries = (int)pic.entries.size(); pp.filter_type = pic.filter_type; pp.sharpness = pic.sharpness; pp.filtered = pic.filtered;
            pp.mbs = pic.mbs.data(); pp.entries = entries.get();
            memcpy(pp.dq, pic.dq, sizeof pp.dq);
            if (!pic.tag.key) {
                pp.inter = 1; pp.interp = pic.tag.version == 0 ? 0 : 1; pp.n_intra = pic.intra_mbs; pp.n_split = (int)pic.split.size(); pp.split = spl.get();
                for (int k = 0; k < 3; k++) pp.ref[k] = ref[k] && ref[k]->W == W && ref[k]->H == H ? ref[k]->p.get() : nullptr;
            }
            vp8_inter_host(pp);
            vp8_reconstruct_host(pp);
            vp8_filter_host(pp);
            if (pic.tag.key) ref[0] = ref[1] = ref[2] = cur;
            else {
                const auto last = ref[0], gold = ref[1], alt = ref[2];
                if (pic.copy_to_alt == 1) ref[2] = last; else if (pic.copy_to_alt == 2) ref[2] = gold;
                if (pic.copy_to_golden == 1) ref[1] = last; else if (pic.copy_to_golden == 2) ref[1] = alt;
                if (pic.refresh_golden) ref[1] = cur;
                if (pic.refresh_alt) ref[2] = cur;
                if (pic.refresh_last) ref[0] = cur;
            }
            pictures++;
        };
        for (size_t o = 0; o < d.size();) { const size_t k = std::min(d.size() - o, (size_t)(t % 3 == 0 ? d.size() : 1 + rng() % 300)); sp.feed(d.data() + o, k, sink); o += k; }
        sp.flush(sink);
    }
    printf("%s: %d trials, %ld pictures decoded, %ld inter frames, %ld damaged, %ld refused, %ld empty frames\n", bad ? "FAILED" : "ok", trials, pictures, inter, damaged, refused, empty);
    return bad;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: vp8_inter_asan <seed> <trials> [stream.ivf]\n"); return 2; }
    std::mt19937 rng((unsigned)atoi(argv[1]));
    const int trials = atoi(argv[2]);
    return argc > 3 ? fuzz_stream(rng, trials, argv[3]) : random_lists(rng, trials);
}
