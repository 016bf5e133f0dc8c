// jmcodec_amd/csrc/deblock_packed.h -- the edge filters of H.264 8.7.2.3 / 8.7.2.4 as the deblocking kernels run them: the luma filter on PACKED
// 16-bit pairs and the branch-free chroma filter of the LDS wavefront (deblock_device.h: k_deblock_band, k_chain, k_chain_i), and the scalar pair of the
// spin-wait kernel (kernels.hip: k_deblock).
//
// Every function is __host__ __device__: on the device the instructions are what they were when these functions lived in deblock_device.h and
// kernels.hip; on the host v_sad_u8, v_alignbit_b32, the packed 16-bit arithmetic and the wave ballot (of one lane) are restated in plain C++, so that
// tests/test_deblock_packed.py checks all four forms against a literal, clause-ordered restatement of 8.7.2.3 / 8.7.2.4 WITHOUT a GPU
// (tests/native/deblock_packed_check.cpp).  On the GPU the analytic and oracle-parity tests run the same functions with the real instructions.
//
// Part of the replacement for cuvidDecodePicture (nv_dec/nv_dec.cpp:33-41 of the reference).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "kernel_common.h"     // clip3, clip1, iabs
#define JM_DB_HD __host__ __device__ __forceinline__
#else
#define JM_DB_HD static inline
#endif

namespace jmamd {

#if !defined(__HIPCC__)
// host builds of the checks have no kernel_common.h (device code): the same three helpers
JM_DB_HD int clip3(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }
JM_DB_HD int clip1(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
JM_DB_HD int iabs(int v) { return v < 0 ? -v : v; }
#endif

#if defined(__HIPCC__)
typedef short s2 __attribute__((ext_vector_type(2)));
JM_DB_HD s2 pmin(s2 a, s2 b) { return __builtin_elementwise_min(a, b); }
JM_DB_HD s2 pmax(s2 a, s2 b) { return __builtin_elementwise_max(a, b); }
JM_DB_HD s2 as_s2(uint32_t v) { return __builtin_bit_cast(s2, v); }
JM_DB_HD uint32_t as_u(s2 v) { return __builtin_bit_cast(uint32_t, v); }
#else
// ---- the packed 16-bit arithmetic in plain C++ (CDNA3 instruction set manual, V_PK_*_I16 / U16) ----
// two 16-bit lanes, low half first; arithmetic wraps at 16 bits, >> is arithmetic, as the v_pk_* instructions do
struct s2 { int16_t x, y; };
JM_DB_HD s2 mk_s2(int x, int y) { return s2{(int16_t)(uint16_t)(x & 0xffff), (int16_t)(uint16_t)(y & 0xffff)}; }
JM_DB_HD s2 operator+(s2 a, s2 b) { return mk_s2(a.x + b.x, a.y + b.y); }
JM_DB_HD s2 operator-(s2 a, s2 b) { return mk_s2(a.x - b.x, a.y - b.y); }
JM_DB_HD s2 operator-(s2 a) { return mk_s2(-a.x, -a.y); }
JM_DB_HD s2 operator<<(s2 a, int n) { return mk_s2((int)((uint32_t)(uint16_t)a.x << n), (int)((uint32_t)(uint16_t)a.y << n)); }
JM_DB_HD s2 operator>>(s2 a, int n) { return mk_s2(a.x >> n, a.y >> n); }
JM_DB_HD s2 pmin(s2 a, s2 b) { return s2{a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y}; }
JM_DB_HD s2 pmax(s2 a, s2 b) { return s2{a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y}; }
JM_DB_HD s2 as_s2(uint32_t v) { return mk_s2((int)(v & 0xffffu), (int)(v >> 16)); }
JM_DB_HD uint32_t as_u(s2 v) { return (uint32_t)(uint16_t)v.x | ((uint32_t)(uint16_t)v.y << 16); }
#endif
#if defined(__HIP_DEVICE_COMPILE__)
JM_DB_HD uint32_t sad_u8(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_sad_u8(a, b, c); }
JM_DB_HD uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbit(hi, lo, sh); }
JM_DB_HD bool any_lane(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0; }
#else
// ---- the three instructions in plain C++ (V_SAD_U8, V_ALIGNBIT_B32; the ballot of ONE lane is its own condition) ----
JM_DB_HD uint32_t sad_u8(uint32_t a, uint32_t b, uint32_t c) {
    for (int k = 0; k < 4; k++) { const int x = (int)((a >> (8 * k)) & 255), y = (int)((b >> (8 * k)) & 255); c += (uint32_t)(x < y ? y - x : x - y); }
    return c;
}
JM_DB_HD uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31)); }
JM_DB_HD bool any_lane(bool c) { return c; }
#endif

// ------------------------------------------------------------------------------------------
// sample filters on register arrays
// ------------------------------------------------------------------------------------------
// s[0..7] = p3 p2 p1 p0 q0 q1 q2 q3; bsw = bS | tC0 << 3.  Written without divergent branches: the two filters of 8.7.2.3 / 8.7.2.4
// are computed for every lane and selected, and the only branches are wave-uniform (nothing to filter / no lane with bS = 4).  The
// branchy form cost ~10 exec-mask regions and, in the horizontal pass, ~110 register copies at the joins per edge.
// |a - b| of two samples (0..255, upper bytes zero): one v_sad_u8 instead of sub / neg / max
JM_DB_HD int adiff(int a, int b) { return (int)sad_u8((unsigned)a, (unsigned)b, 0u); }
JM_DB_HD int sel(bool c, int a, int b) { return c ? a : b; }      // operands are evaluated by the caller: a v_cndmask, never a branch
// ---- the luma edge filter on PACKED 16-bit pairs (round 3) ----
// One 32-bit register holds the sample i of the p side in its low half and the sample i of the q side in its high half: A = (p0 | q0 << 16),
// B = (p1 | q1), C = (p2 | q2), D = (p3 | q3).  The two sides of 8.7.2.3 / 8.7.2.4 are mirror images, so every side-wise quantity (|p1 - p0| and
// |q1 - q0|, ap and aq, p1' and q1', the strong filter's three outputs per side) is ONE v_pk_* instruction instead of two scalar ones, conditions
// become masks ((x - limit) >> 15 per half) and selects become bitwise blends: ~60 vector instructions for the normal filter where the scalar
// form needed ~100, and no int <-> bool conversions.  Same arithmetic, value for value (tests/test_deblock_packed.py: every bS, every alpha / beta /
// tC0 of Tables 8-16 / 8-17, octets on every threshold, against the clause).
JM_DB_HD s2 splat(int v) { return as_s2((uint32_t)v | ((uint32_t)v << 16)); }      // 0 <= v < 65536
JM_DB_HD s2 swp(s2 v) { const uint32_t u = as_u(v); return as_s2(alignbit(u, u, 16)); }
JM_DB_HD s2 pabs(s2 v) { return pmax(v, -v); }
JM_DB_HD s2 blend(uint32_t m, s2 a, s2 b) { return as_s2((as_u(a) & m) | (as_u(b) & ~m)); }      // m: all ones / all zeros per half
// A, B, C are updated in place (D = p3 | q3 is only read); bsw = bS | tC0 << 3
JM_DB_HD void flt_luma(s2 &A, s2 &B, s2 &C, const s2 D, int bsw, int alpha, int beta) {
    const int bS = bsw & 7, tc0 = bsw >> 3;
    const s2 As = swp(A), Bs = swp(B);
    const s2 beta2 = splat(beta);
    const s2 d10 = pabs(B - A), dpq = pabs(As - A);                       // (|p1 - p0| , |q1 - q0|), |p0 - q0| in both halves
    const s2 m10 = (d10 - beta2) >> 15, mpq = (dpq - splat(alpha)) >> 15;
    const uint32_t on = as_u(m10) & as_u(swp(m10)) & as_u(mpq) & (bS ? 0xffffffffu : 0u);      // filterSamplesFlag, the same in both halves
    if (!any_lane(on != 0)) return;
    const s2 m20 = (pabs(C - A) - beta2) >> 15;                           // (ap , aq) as masks
    const int tc = tc0 + (int)(as_u(m20) & 1u) + (int)(as_u(m20) >> 31);
    const s2 t = ((As - A) << 2) + (B - Bs) + splat(4);                    // low half: ((q0 - p0) << 2) + (p1 - q1) + 4
    const int dl = clip3(-tc, tc, (int)(short)(as_u(t) & 0xffffu) >> 3);
    const s2 dd = as_s2(((uint32_t)dl & 0xffffu) | ((uint32_t)(-dl) << 16));       // (+delta , -delta)
    const s2 nA = pmin(pmax(A + dd, splat(0)), splat(255));
    const s2 avg = as_s2((as_u(A + As + splat(1)) >> 1) & 0x7fff7fffu);     // (p0 + q0 + 1) >> 1 in both halves
    const s2 tcs = splat(tc0);
    const s2 tt = pmin(pmax((C + avg - (B << 1)) >> 1, -tcs), tcs);
    const s2 nB = B + as_s2(as_u(tt) & as_u(m20));                        // p1' only with ap, q1' only with aq
    const uint32_t nrm = on & (bS < 4 ? 0xffffffffu : 0u);
    s2 rA = blend(nrm, nA, A), rB = blend(nrm, nB, B), rC = C;
    const uint32_t st = on & (bS >= 4 ? 0xffffffffu : 0u);
    if (any_lane(st != 0)) {
        const s2 msg = (dpq - splat((alpha >> 2) + 2)) >> 15;
        const uint32_t sm = st & as_u(m20) & as_u(msg);                    // the strong filter, per side
        const s2 S0 = (C + ((B + A + As) << 1) + Bs + splat(4)) >> 3;
        const s2 S1 = (C + B + A + As + splat(2)) >> 2;
        const s2 S2 = ((D << 1) + C + (C << 1) + B + A + As + splat(4)) >> 3;
        const s2 W0 = ((B << 1) + A + Bs + splat(2)) >> 2;
        rA = blend(sm, S0, blend(st, W0, rA)); rB = blend(sm, S1, rB); rC = blend(sm, S2, rC);
    }
    A = rA; B = rB; C = rC;
}
// chroma: p1 p0 q0 q1 by reference
JM_DB_HD void flt_chroma(int p1, int &p0, int &q0, int q1, int bsw, int alpha, int beta) {
    const int bS = bsw & 7, tc = (bsw >> 3) + 1;
    const bool on = ((int)(bS != 0) & (int)(adiff(p0, q0) < alpha) & (int)(adiff(p1, p0) < beta) & (int)(adiff(q1, q0) < beta)) != 0;
    const int delta = clip3(-tc, tc, (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3);
    const int n_p0 = clip1(p0 + delta), n_q0 = clip1(q0 - delta), w_p0 = (2 * p1 + p0 + q1 + 2) >> 2, w_q0 = (2 * q1 + q0 + p1 + 2) >> 2;
    p0 = sel(on, sel(bS < 4, n_p0, w_p0), p0); q0 = sel(on, sel(bS < 4, n_q0, w_q0), q0);
}

// ------------------------------------------------------------------------------------------
// the scalar pair of k_deblock (kernels.hip): the caller skips bS 0; tc0_row = the three tC0 of indexA (Table 8-17)
// ------------------------------------------------------------------------------------------
// filter one line across an edge; s[0..7] = p3 p2 p1 p0 q0 q1 q2 q3 (luma) in registers
JM_DB_HD void filter_luma(int *s, int bS, int alpha, int beta, const uint8_t *tc0_row) {
    int p3 = s[0], p2 = s[1], p1 = s[2], p0 = s[3], q0 = s[4], q1 = s[5], q2 = s[6], q3 = s[7];
    if (!(iabs(p0 - q0) < alpha && iabs(p1 - p0) < beta && iabs(q1 - q0) < beta)) return;
    int ap = iabs(p2 - p0) < beta, aq = iabs(q2 - q0) < beta;
    if (bS < 4) {
        int tc0 = tc0_row[bS - 1], tc = tc0 + ap + aq;
        int delta = clip3(-tc, tc, (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3);
        s[3] = clip1(p0 + delta); s[4] = clip1(q0 - delta);
        if (ap) s[2] = p1 + clip3(-tc0, tc0, (p2 + ((p0 + q0 + 1) >> 1) - (p1 << 1)) >> 1);
        if (aq) s[5] = q1 + clip3(-tc0, tc0, (q2 + ((p0 + q0 + 1) >> 1) - (q1 << 1)) >> 1);
    } else {
        bool strong = iabs(p0 - q0) < ((alpha >> 2) + 2);
        if (ap && strong) { s[3] = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3; s[2] = (p2 + p1 + p0 + q0 + 2) >> 2;
            s[1] = (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3; }
        else s[3] = (2 * p1 + p0 + q1 + 2) >> 2;
        if (aq && strong) { s[4] = (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3; s[5] = (p0 + q0 + q1 + q2 + 2) >> 2;
            s[6] = (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3; }
        else s[4] = (2 * q1 + q0 + p1 + 2) >> 2;
    }
}
// chroma: s[0..3] = p1 p0 q0 q1
JM_DB_HD void filter_chroma(int *s, int bS, int alpha, int beta, const uint8_t *tc0_row) {
    int p1 = s[0], p0 = s[1], q0 = s[2], q1 = s[3];
    if (!(iabs(p0 - q0) < alpha && iabs(p1 - p0) < beta && iabs(q1 - q0) < beta)) return;
    if (bS < 4) {
        int tc = tc0_row[bS - 1] + 1;
        int delta = clip3(-tc, tc, (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3);
        s[1] = clip1(p0 + delta); s[2] = clip1(q0 - delta);
    } else { s[1] = (2 * p1 + p0 + q1 + 2) >> 2; s[2] = (2 * q1 + q0 + p1 + 2) >> 2; }
}

}  // namespace jmamd
