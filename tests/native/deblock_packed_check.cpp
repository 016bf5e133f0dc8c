// tests/native/deblock_packed_check.cpp -- host build of jmcodec_amd/csrc/deblock_packed.h (the H.264 edge filters as the deblocking kernels run them)
// behind a C ABI, beside a literal, clause-ordered restatement of 8.7.2.2 (filterSamplesFlag), 8.7.2.3 (bS < 4) and 8.7.2.4 (bS = 4) that also counts
// which paths of the clause a sweep took.  tests/test_deblock_packed.py drives both over the same lines.  Test infrastructure only.
//
// A line is p3 p2 p1 p0 q0 q1 q2 q3 (luma, 8 bytes) or p1 p0 q0 q1 (chroma, 4 bytes); per line: bS, alpha, beta and the three tC0 of indexA (Table 8-17).
#include "../../jmcodec_amd/csrc/deblock_packed.h"
using namespace jmamd;

namespace {
inline int Abs(int v) { return v < 0 ? -v : v; }
inline int Clip3(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }

// path counters of the luma restatement
enum { L_ON_BS1 = 0, L_ON_BS2, L_ON_BS3, L_ON_BS4, L_OFF_ALPHA_ONLY, L_OFF_BETA_P_ONLY, L_OFF_BETA_Q_ONLY, L_AP0_AQ0, L_AP0_AQ1, L_AP1_AQ0, L_AP1_AQ1,
       L_DELTA_CLIP_POS, L_DELTA_CLIP_NEG, L_DELTA_UNCLIPPED, L_DELTA_AT_POS_TC, L_DELTA_AT_NEG_TC, L_DELTA_AT_POS_TC1, L_DELTA_AT_NEG_TC1,
       L_CLIP1_AT_0, L_CLIP1_AT_255, L_SUM_IS_0, L_SUM_IS_255, L_STRONG_BOTH, L_STRONG_P, L_STRONG_Q, L_STRONG_NONE, L_BS0, L_P1_CLIPPED, L_P1_UNCLIPPED,
       L_COUNT };
enum { C_LT4_ON = 0, C_LT4_OFF, C_4_ON, C_4_OFF, C_DELTA_CLIP_POS, C_DELTA_CLIP_NEG, C_DELTA_UNCLIPPED, C_CLIP1_AT_0, C_CLIP1_AT_255, C_BS0, C_COUNT };

inline int Clip1Counted(int v, uint64_t *cnt, int at0, int at255, int is0, int is255) {
    if (v < 0) cnt[at0]++; else if (v > 255) cnt[at255]++;
    if (is0 >= 0) { if (v == 0) cnt[is0]++; else if (v == 255) cnt[is255]++; }
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}
}  // namespace

extern "C" {

int dbp_luma_counters(void) { return L_COUNT; }
int dbp_chroma_counters(void) { return C_COUNT; }

// ---- the clause, luma (chromaStyleFilteringFlag = 0) ----
void dbp_luma_literal(int n, const uint8_t *in, const uint8_t *bS_, const uint8_t *alpha_, const uint8_t *beta_, const uint8_t *tc0_, uint8_t *out,
                      uint64_t *cnt) {
    for (int i = 0; i < n; i++) {
        const int p3 = in[8 * i], p2 = in[8 * i + 1], p1 = in[8 * i + 2], p0 = in[8 * i + 3], q0 = in[8 * i + 4], q1 = in[8 * i + 5], q2 = in[8 * i + 6],
                  q3 = in[8 * i + 7];
        const int bS = bS_[i], alpha = alpha_[i], beta = beta_[i];
        int pp0 = p0, pp1 = p1, pp2 = p2, qq0 = q0, qq1 = q1, qq2 = q2;
        // 8.7.2.2: filterSamplesFlag = ( bS != 0 && Abs( p0 - q0 ) < alpha && Abs( p1 - p0 ) < beta && Abs( q1 - q0 ) < beta )        (8-468)
        const bool ta = Abs(p0 - q0) < alpha, tp = Abs(p1 - p0) < beta, tq = Abs(q1 - q0) < beta;
        const bool filterSamplesFlag = bS != 0 && ta && tp && tq;
        if (bS == 0) cnt[L_BS0]++;
        else if (!filterSamplesFlag) {
            if (!ta && tp && tq) cnt[L_OFF_ALPHA_ONLY]++;
            if (ta && !tp && tq) cnt[L_OFF_BETA_P_ONLY]++;
            if (ta && tp && !tq) cnt[L_OFF_BETA_Q_ONLY]++;
        } else cnt[L_ON_BS1 + bS - 1]++;
        if (filterSamplesFlag && bS < 4) {
            // 8.7.2.3
            const int tC0 = tc0_[3 * i + bS - 1];                                         // Table 8-17, column bS
            const int ap = Abs(p2 - p0), aq = Abs(q2 - q0);                                // (8-471), (8-472)
            const int tC = tC0 + ((ap < beta) ? 1 : 0) + ((aq < beta) ? 1 : 0);            // (8-473)
            const int raw = (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3;
            const int delta = Clip3(-tC, tC, raw);                                         // (8-475)
            cnt[L_AP0_AQ0 + 2 * (ap < beta) + (aq < beta)]++;
            if (raw > tC) cnt[L_DELTA_CLIP_POS]++; else if (raw < -tC) cnt[L_DELTA_CLIP_NEG]++; else cnt[L_DELTA_UNCLIPPED]++;
            if (tC > 0) { if (raw == tC) cnt[L_DELTA_AT_POS_TC]++; if (raw == -tC) cnt[L_DELTA_AT_NEG_TC]++; if (raw == tC + 1) cnt[L_DELTA_AT_POS_TC1]++;
                if (raw == -(tC + 1)) cnt[L_DELTA_AT_NEG_TC1]++; }
            pp0 = Clip1Counted(p0 + delta, cnt, L_CLIP1_AT_0, L_CLIP1_AT_255, L_SUM_IS_0, L_SUM_IS_255);      // (8-476)
            qq0 = Clip1Counted(q0 - delta, cnt, L_CLIP1_AT_0, L_CLIP1_AT_255, L_SUM_IS_0, L_SUM_IS_255);      // (8-477)
            if (ap < beta) { const int r = (p2 + ((p0 + q0 + 1) >> 1) - (p1 << 1)) >> 1; pp1 = p1 + Clip3(-tC0, tC0, r);      // (8-478)
                cnt[(r > tC0 || r < -tC0) ? L_P1_CLIPPED : L_P1_UNCLIPPED]++; }
            else pp1 = p1;                                                                                     // (8-479)
            if (aq < beta) { const int r = (q2 + ((p0 + q0 + 1) >> 1) - (q1 << 1)) >> 1; qq1 = q1 + Clip3(-tC0, tC0, r);      // (8-480)
                cnt[(r > tC0 || r < -tC0) ? L_P1_CLIPPED : L_P1_UNCLIPPED]++; }
            else qq1 = q1;                                                                                     // (8-481)
            pp2 = p2; qq2 = q2;                                                                                // (8-482), (8-483)
        } else if (filterSamplesFlag) {
            // 8.7.2.4
            const int ap = Abs(p2 - p0), aq = Abs(q2 - q0);
            const bool sp = ap < beta && Abs(p0 - q0) < ((alpha >> 2) + 2), sq = aq < beta && Abs(p0 - q0) < ((alpha >> 2) + 2);
            cnt[sp && sq ? L_STRONG_BOTH : (sp ? L_STRONG_P : (sq ? L_STRONG_Q : L_STRONG_NONE))]++;
            if (sp) { pp0 = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3;                 // (8-485)
                pp1 = (p2 + p1 + p0 + q0 + 2) >> 2;                                        // (8-486)
                pp2 = (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3; }                         // (8-487)
            else { pp0 = (2 * p1 + p0 + q1 + 2) >> 2; pp1 = p1; pp2 = p2; }                // (8-488) .. (8-490)
            if (sq) { qq0 = (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3;                 // (8-492)
                qq1 = (p0 + q0 + q1 + q2 + 2) >> 2;                                        // (8-493)
                qq2 = (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3; }                         // (8-494)
            else { qq0 = (2 * q1 + q0 + p1 + 2) >> 2; qq1 = q1; qq2 = q2; }                // (8-495) .. (8-497)
        }
        uint8_t *o = out + 8 * i;
        o[0] = (uint8_t)p3; o[1] = (uint8_t)pp2; o[2] = (uint8_t)pp1; o[3] = (uint8_t)pp0; o[4] = (uint8_t)qq0; o[5] = (uint8_t)qq1; o[6] = (uint8_t)qq2;
        o[7] = (uint8_t)q3;
    }
}

// ---- the clause, chroma (chromaStyleFilteringFlag = 1, chromaEdgeFlag = 1) ----
void dbp_chroma_literal(int n, const uint8_t *in, const uint8_t *bS_, const uint8_t *alpha_, const uint8_t *beta_, const uint8_t *tc0_, uint8_t *out,
                        uint64_t *cnt) {
    for (int i = 0; i < n; i++) {
        const int p1 = in[4 * i], p0 = in[4 * i + 1], q0 = in[4 * i + 2], q1 = in[4 * i + 3];
        const int bS = bS_[i], alpha = alpha_[i], beta = beta_[i];
        int pp0 = p0, qq0 = q0;
        const bool filterSamplesFlag = bS != 0 && Abs(p0 - q0) < alpha && Abs(p1 - p0) < beta && Abs(q1 - q0) < beta;      // (8-468)
        if (bS == 0) cnt[C_BS0]++;
        else cnt[(bS < 4 ? C_LT4_ON : C_4_ON) + (filterSamplesFlag ? 0 : 1)]++;
        if (filterSamplesFlag && bS < 4) {
            const int tC0 = tc0_[3 * i + bS - 1];
            const int tC = tC0 + 1;                                                        // (8-474)
            const int raw = (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3;
            const int delta = Clip3(-tC, tC, raw);                                         // (8-475)
            if (raw > tC) cnt[C_DELTA_CLIP_POS]++; else if (raw < -tC) cnt[C_DELTA_CLIP_NEG]++; else cnt[C_DELTA_UNCLIPPED]++;
            pp0 = Clip1Counted(p0 + delta, cnt, C_CLIP1_AT_0, C_CLIP1_AT_255, -1, -1);     // (8-476)
            qq0 = Clip1Counted(q0 - delta, cnt, C_CLIP1_AT_0, C_CLIP1_AT_255, -1, -1);     // (8-477)
        } else if (filterSamplesFlag) {
            pp0 = (2 * p1 + p0 + q1 + 2) >> 2;                                             // (8-488)
            qq0 = (2 * q1 + q0 + p1 + 2) >> 2;                                             // (8-495)
        }
        uint8_t *o = out + 4 * i;
        o[0] = (uint8_t)p1; o[1] = (uint8_t)pp0; o[2] = (uint8_t)qq0; o[3] = (uint8_t)q1;
    }
}

// ---- the product's forms.  bsw = bS | tC0 << 3 with tC0 = 0 for bS 0 and 4, as k_deblock_prep (deblock_lds.hip) writes it ----
static inline int bsw_of(int bS, const uint8_t *tc0row) { return bS | ((bS >= 1 && bS <= 3 ? tc0row[bS - 1] : 0) << 3); }

void dbp_luma_packed(int n, const uint8_t *in, const uint8_t *bS_, const uint8_t *alpha_, const uint8_t *beta_, const uint8_t *tc0_, uint8_t *out) {
    for (int i = 0; i < n; i++) {
        const uint8_t *s = in + 8 * i;
        s2 A = as_s2(s[3] | (uint32_t)s[4] << 16), B = as_s2(s[2] | (uint32_t)s[5] << 16), C = as_s2(s[1] | (uint32_t)s[6] << 16);
        const s2 D = as_s2(s[0] | (uint32_t)s[7] << 16);
        flt_luma(A, B, C, D, bsw_of(bS_[i], tc0_ + 3 * i), alpha_[i], beta_[i]);
        uint8_t *o = out + 8 * i;
        // the kernels store the low byte of each half (luma_mb: (uint8_t)as_u(X), (uint8_t)(as_u(X) >> 16)); a half outside 0..255 would show here
        // as a wrong byte, and is reported through dbp_luma_packed's return value as well
        o[0] = (uint8_t)as_u(D); o[1] = (uint8_t)as_u(C); o[2] = (uint8_t)as_u(B); o[3] = (uint8_t)as_u(A);
        o[4] = (uint8_t)(as_u(A) >> 16); o[5] = (uint8_t)(as_u(B) >> 16); o[6] = (uint8_t)(as_u(C) >> 16); o[7] = (uint8_t)(as_u(D) >> 16);
    }
}
// number of lines after which a 16-bit half of A, B or C is not a sample value (the v_perm stores of luma_mb's vertical pass take whole bytes too)
int dbp_luma_packed_out_of_range(int n, const uint8_t *in, const uint8_t *bS_, const uint8_t *alpha_, const uint8_t *beta_, const uint8_t *tc0_) {
    int bad = 0;
    for (int i = 0; i < n; i++) {
        const uint8_t *s = in + 8 * i;
        s2 A = as_s2(s[3] | (uint32_t)s[4] << 16), B = as_s2(s[2] | (uint32_t)s[5] << 16), C = as_s2(s[1] | (uint32_t)s[6] << 16);
        const s2 D = as_s2(s[0] | (uint32_t)s[7] << 16);
        flt_luma(A, B, C, D, bsw_of(bS_[i], tc0_ + 3 * i), alpha_[i], beta_[i]);
        if ((as_u(A) | as_u(B) | as_u(C)) & 0xff00ff00u) bad++;
    }
    return bad;
}
void dbp_chroma_packed(int n, const uint8_t *in, const uint8_t *bS_, const uint8_t *alpha_, const uint8_t *beta_, const uint8_t *tc0_, uint8_t *out) {
    for (int i = 0; i < n; i++) {
        int p0 = in[4 * i + 1], q0 = in[4 * i + 2];
        flt_chroma(in[4 * i], p0, q0, in[4 * i + 3], bsw_of(bS_[i], tc0_ + 3 * i), alpha_[i], beta_[i]);
        out[4 * i] = in[4 * i]; out[4 * i + 1] = (uint8_t)p0; out[4 * i + 2] = (uint8_t)q0; out[4 * i + 3] = in[4 * i + 3];
    }
}
// the scalar pair of k_deblock: deblock_mb (kernels.hip) skips bS 0 before it calls them, and so does this
void dbp_luma_scalar(int n, const uint8_t *in, const uint8_t *bS_, const uint8_t *alpha_, const uint8_t *beta_, const uint8_t *tc0_, uint8_t *out) {
    for (int i = 0; i < n; i++) {
        int s[8];
        for (int k = 0; k < 8; k++) s[k] = in[8 * i + k];
        if (bS_[i]) filter_luma(s, bS_[i], alpha_[i], beta_[i], tc0_ + 3 * i);
        for (int k = 0; k < 8; k++) out[8 * i + k] = (uint8_t)s[k];
    }
}
void dbp_chroma_scalar(int n, const uint8_t *in, const uint8_t *bS_, const uint8_t *alpha_, const uint8_t *beta_, const uint8_t *tc0_, uint8_t *out) {
    for (int i = 0; i < n; i++) {
        int s[4];
        for (int k = 0; k < 4; k++) s[k] = in[4 * i + k];
        if (bS_[i]) filter_chroma(s, bS_[i], alpha_[i], beta_[i], tc0_ + 3 * i);
        for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)s[k];
    }
}

}  // extern "C"
