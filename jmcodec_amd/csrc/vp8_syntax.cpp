// jmcodec_amd/csrc/vp8_syntax.cpp -- VP8 (codec_type 5): frame header, modes, vectors and tokens into the job list (vp8_syntax.h, vp8_jobs.h).
// RFC 6386 sections 9 (frame header), 11 (key-frame modes), 13 (tokens), 14.1 (quantiser), and for inter frames (option vp8_inter) 9.7, 9.10, 9.11, 16
// (modes and vectors of inter frames), 17 (vector decoding); what is accepted and refused: INTEGRATION.md "VP8".
#include "vp8_syntax.h"
#include <algorithm>
#include <cstdio>
#include <cstring>

namespace jmamd {

// ---- tables -------------------------------------------------------------------------------------------------------------------------------------
const uint8_t kVp8DcQ[128] = {
    4,   5,   6,   7,   8,   9,   10,  10,  11,  12,  13,  14,  15,  16,  17,  17,  18,  19,  20,  20,  21,  21,  22,  22,  23,  23,  24,  25,  25,  26,  27,  28,
    29,  30,  31,  32,  33,  34,  35,  36,  37,  37,  38,  39,  40,  41,  42,  43,  44,  45,  46,  46,  47,  48,  49,  50,  51,  52,  53,  54,  55,  56,  57,  58,
    59,  60,  61,  62,  63,  64,  65,  66,  67,  68,  69,  70,  71,  72,  73,  74,  75,  76,  76,  77,  78,  79,  80,  81,  82,  83,  84,  85,  86,  87,  88,  89,
    91,  93,  95,  96,  98,  100, 101, 102, 104, 106, 108, 110, 112, 114, 116, 118, 122, 124, 126, 128, 130, 132, 134, 136, 138, 140, 143, 145, 148, 151, 154, 157};
const uint16_t kVp8AcQ[128] = {
    4,   5,   6,   7,   8,   9,   10,  11,  12,  13,  14,  15,  16,  17,  18,  19,  20,  21,  22,  23,  24,  25,  26,  27,  28,  29,  30,  31,  32,  33,  34,  35,
    36,  37,  38,  39,  40,  41,  42,  43,  44,  45,  46,  47,  48,  49,  50,  51,  52,  53,  54,  55,  56,  57,  58,  60,  62,  64,  66,  68,  70,  72,  74,  76,
    78,  80,  82,  84,  86,  88,  90,  92,  94,  96,  98,  100, 102, 104, 106, 108, 110, 112, 114, 116, 119, 122, 125, 128, 131, 134, 137, 140, 143, 146, 149, 152,
    155, 158, 161, 164, 167, 170, 173, 177, 181, 185, 189, 193, 197, 201, 205, 209, 213, 217, 221, 225, 229, 234, 239, 245, 249, 254, 259, 264, 269, 274, 279, 284};

#define H 128
const uint8_t kVp8CoefProbs[4][8][3][11] = {
    {   // block type 0: luma after Y2 (position 0 is never coded: band 0 is unused)
        {{H, H, H, H, H, H, H, H, H, H, H}, {H, H, H, H, H, H, H, H, H, H, H}, {H, H, H, H, H, H, H, H, H, H, H}},
        {{253, 136, 254, 255, 228, 219, H, H, H, H, H}, {189, 129, 242, 255, 227, 213, 255, 219, H, H, H}, {106, 126, 227, 252, 214, 209, 255, 255, H, H, H}},
        {{1, 98, 248, 255, 236, 226, 255, 255, H, H, H}, {181, 133, 238, 254, 221, 234, 255, 154, H, H, H}, {78, 134, 202, 247, 198, 180, 255, 219, H, H, H}},
        {{1, 185, 249, 255, 243, 255, H, H, H, H, H}, {184, 150, 247, 255, 236, 224, H, H, H, H, H}, {77, 110, 216, 255, 236, 230, H, H, H, H, H}},
        {{1, 101, 251, 255, 241, 255, H, H, H, H, H}, {170, 139, 241, 252, 236, 209, 255, 255, H, H, H}, {37, 116, 196, 243, 228, 255, 255, 255, H, H, H}},
        {{1, 204, 254, 255, 245, 255, H, H, H, H, H}, {207, 160, 250, 255, 238, H, H, H, H, H, H}, {102, 103, 231, 255, 211, 171, H, H, H, H, H}},
        {{1, 152, 252, 255, 240, 255, H, H, H, H, H}, {177, 135, 243, 255, 234, 225, H, H, H, H, H}, {80, 129, 211, 255, 194, 224, H, H, H, H, H}},
        {{1, 1, 255, H, H, H, H, H, H, H, H}, {246, 1, 255, H, H, H, H, H, H, H, H}, {255, H, H, H, H, H, H, H, H, H, H}},
    },
    {   // block type 1: Y2
        {{198, 35, 237, 223, 193, 187, 162, 160, 145, 155, 62}, {131, 45, 198, 221, 172, 176, 220, 157, 252, 221, 1}, {68, 47, 146, 208, 149, 167, 221, 162, 255, 223, H}},
        {{1, 149, 241, 255, 221, 224, 255, 255, H, H, H}, {184, 141, 234, 253, 222, 220, 255, 199, H, H, H}, {81, 99, 181, 242, 176, 190, 249, 202, 255, 255, H}},
        {{1, 129, 232, 253, 214, 197, 242, 196, 255, 255, H}, {99, 121, 210, 250, 201, 198, 255, 202, H, H, H}, {23, 91, 163, 242, 170, 187, 247, 210, 255, 255, H}},
        {{1, 200, 246, 255, 234, 255, H, H, H, H, H}, {109, 178, 241, 255, 231, 245, 255, 255, H, H, H}, {44, 130, 201, 253, 205, 192, 255, 255, H, H, H}},
        {{1, 132, 239, 251, 219, 209, 255, 165, H, H, H}, {94, 136, 225, 251, 218, 190, 255, 255, H, H, H}, {22, 100, 174, 245, 186, 161, 255, 199, H, H, H}},
        {{1, 182, 249, 255, 232, 235, H, H, H, H, H}, {124, 143, 241, 255, 227, 234, H, H, H, H, H}, {35, 77, 181, 251, 193, 211, 255, 205, H, H, H}},
        {{1, 157, 247, 255, 236, 231, 255, 255, H, H, H}, {121, 141, 235, 255, 225, 227, 255, 255, H, H, H}, {45, 99, 188, 251, 195, 217, 255, 224, H, H, H}},
        {{1, 1, 251, 255, 213, 255, H, H, H, H, H}, {203, 1, 248, 255, 255, H, H, H, H, H, H}, {137, 1, 177, 255, 224, 255, H, H, H, H, H}},
    },
    {   // block type 2: chroma
        {{253, 9, 248, 251, 207, 208, 255, 192, H, H, H}, {175, 13, 224, 243, 193, 185, 249, 198, 255, 255, H}, {73, 17, 171, 221, 161, 179, 236, 167, 255, 234, H}},
        {{1, 95, 247, 253, 212, 183, 255, 255, H, H, H}, {239, 90, 244, 250, 211, 209, 255, 255, H, H, H}, {155, 77, 195, 248, 188, 195, 255, 255, H, H, H}},
        {{1, 24, 239, 251, 218, 219, 255, 205, H, H, H}, {201, 51, 219, 255, 196, 186, H, H, H, H, H}, {69, 46, 190, 239, 201, 218, 255, 228, H, H, H}},
        {{1, 191, 251, 255, 255, H, H, H, H, H, H}, {223, 165, 249, 255, 213, 255, H, H, H, H, H}, {141, 124, 248, 255, 255, H, H, H, H, H, H}},
        {{1, 16, 248, 255, 255, H, H, H, H, H, H}, {190, 36, 230, 255, 236, 255, H, H, H, H, H}, {149, 1, 255, H, H, H, H, H, H, H, H}},
        {{1, 226, 255, H, H, H, H, H, H, H, H}, {247, 192, 255, H, H, H, H, H, H, H, H}, {240, H, 255, H, H, H, H, H, H, H, H}},
        {{1, 134, 252, 255, 255, H, H, H, H, H, H}, {213, 62, 250, 255, 255, H, H, H, H, H, H}, {55, 93, 255, H, H, H, H, H, H, H, H}},
        {{H, H, H, H, H, H, H, H, H, H, H}, {H, H, H, H, H, H, H, H, H, H, H}, {H, H, H, H, H, H, H, H, H, H, H}},
    },
    {   // block type 3: luma with DC
        {{202, 24, 213, 235, 186, 191, 220, 160, 240, 175, 255}, {126, 38, 182, 232, 169, 184, 228, 174, 255, 187, H}, {61, 46, 138, 219, 151, 178, 240, 170, 255, 216, H}},
        {{1, 112, 230, 250, 199, 191, 247, 159, 255, 255, H}, {166, 109, 228, 252, 211, 215, 255, 174, H, H, H}, {39, 77, 162, 232, 172, 180, 245, 178, 255, 255, H}},
        {{1, 52, 220, 246, 198, 199, 249, 220, 255, 255, H}, {124, 74, 191, 243, 183, 193, 250, 221, 255, 255, H}, {24, 71, 130, 219, 154, 170, 243, 182, 255, 255, H}},
        {{1, 182, 225, 249, 219, 240, 255, 224, H, H, H}, {149, 150, 226, 252, 216, 205, 255, 171, H, H, H}, {28, 108, 170, 242, 183, 194, 254, 223, 255, 255, H}},
        {{1, 81, 230, 252, 204, 203, 255, 192, H, H, H}, {123, 102, 209, 247, 188, 196, 255, 233, H, H, H}, {20, 95, 153, 243, 164, 173, 255, 203, H, H, H}},
        {{1, 222, 248, 255, 216, 213, H, H, H, H, H}, {168, 175, 246, 252, 235, 205, 255, 255, H, H, H}, {47, 116, 215, 255, 211, 212, 255, 255, H, H, H}},
        {{1, 121, 236, 253, 212, 214, 255, 255, H, H, H}, {141, 84, 213, 252, 201, 202, 255, 219, H, H, H}, {42, 80, 160, 240, 162, 185, 255, 205, H, H, H}},
        {{1, 1, 255, H, H, H, H, H, H, H, H}, {244, 1, 255, H, H, H, H, H, H, H, H}, {238, 1, 255, H, H, H, H, H, H, H, H}},
    },
};
#undef H

#define F 255
const uint8_t kVp8CoefUpdateProbs[4][8][3][11] = {
    {
        {{F, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
        {{176, 246, F, F, F, F, F, F, F, F, F}, {223, 241, 252, F, F, F, F, F, F, F, F}, {249, 253, 253, F, F, F, F, F, F, F, F}},
        {{F, 244, 252, F, F, F, F, F, F, F, F}, {234, 254, 254, F, F, F, F, F, F, F, F}, {253, F, F, F, F, F, F, F, F, F, F}},
        {{F, 246, 254, F, F, F, F, F, F, F, F}, {239, 253, 254, F, F, F, F, F, F, F, F}, {254, F, 254, F, F, F, F, F, F, F, F}},
        {{F, 248, 254, F, F, F, F, F, F, F, F}, {251, F, 254, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
        {{F, 253, 254, F, F, F, F, F, F, F, F}, {251, 254, 254, F, F, F, F, F, F, F, F}, {254, F, 254, F, F, F, F, F, F, F, F}},
        {{F, 254, 253, F, 254, F, F, F, F, F, F}, {250, F, 254, F, 254, F, F, F, F, F, F}, {254, F, F, F, F, F, F, F, F, F, F}},
        {{F, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
    },
    {
        {{217, F, F, F, F, F, F, F, F, F, F}, {225, 252, 241, 253, F, F, 254, F, F, F, F}, {234, 250, 241, 250, 253, F, 253, 254, F, F, F}},
        {{F, 254, F, F, F, F, F, F, F, F, F}, {223, 254, 254, F, F, F, F, F, F, F, F}, {238, 253, 254, 254, F, F, F, F, F, F, F}},
        {{F, 248, 254, F, F, F, F, F, F, F, F}, {249, 254, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
        {{F, 253, F, F, F, F, F, F, F, F, F}, {247, 254, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
        {{F, 253, 254, F, F, F, F, F, F, F, F}, {252, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
        {{F, 254, 254, F, F, F, F, F, F, F, F}, {253, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
        {{F, 254, 253, F, F, F, F, F, F, F, F}, {250, F, F, F, F, F, F, F, F, F, F}, {254, F, F, F, F, F, F, F, F, F, F}},
        {{F, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
    },
    {
        {{186, 251, 250, F, F, F, F, F, F, F, F}, {234, 251, 244, 254, F, F, F, F, F, F, F}, {251, 251, 243, 253, 254, F, 254, F, F, F, F}},
        {{F, 253, 254, F, F, F, F, F, F, F, F}, {236, 253, 254, F, F, F, F, F, F, F, F}, {251, 253, 253, 254, 254, F, F, F, F, F, F}},
        {{F, 254, 254, F, F, F, F, F, F, F, F}, {254, 254, 254, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
        {{F, 254, F, F, F, F, F, F, F, F, F}, {254, 254, F, F, F, F, F, F, F, F, F}, {254, F, F, F, F, F, F, F, F, F, F}},
        {{F, F, F, F, F, F, F, F, F, F, F}, {254, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
        {{F, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
        {{F, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
        {{F, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
    },
    {
        {{248, F, F, F, F, F, F, F, F, F, F}, {250, 254, 252, 254, F, F, F, F, F, F, F}, {248, 254, 249, 253, F, F, F, F, F, F, F}},
        {{F, 253, 253, F, F, F, F, F, F, F, F}, {246, 253, 253, F, F, F, F, F, F, F, F}, {252, 254, 251, 254, 254, F, F, F, F, F, F}},
        {{F, 254, 252, F, F, F, F, F, F, F, F}, {248, 254, 253, F, F, F, F, F, F, F, F}, {253, F, 254, 254, F, F, F, F, F, F, F}},
        {{F, 251, 254, F, F, F, F, F, F, F, F}, {245, 251, 254, F, F, F, F, F, F, F, F}, {253, 253, 254, F, F, F, F, F, F, F, F}},
        {{F, 251, 253, F, F, F, F, F, F, F, F}, {252, 253, 254, F, F, F, F, F, F, F, F}, {F, 254, F, F, F, F, F, F, F, F, F}},
        {{F, 252, F, F, F, F, F, F, F, F, F}, {249, F, 254, F, F, F, F, F, F, F, F}, {F, F, 254, F, F, F, F, F, F, F, F}},
        {{F, F, 253, F, F, F, F, F, F, F, F}, {250, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
        {{F, F, F, F, F, F, F, F, F, F, F}, {254, F, F, F, F, F, F, F, F, F, F}, {F, F, F, F, F, F, F, F, F, F, F}},
    },
};
#undef F

const uint8_t kVp8KfYmodeProb[4] = {145, 156, 163, 128}, kVp8KfUvModeProb[3] = {142, 114, 183};
// trees: a positive entry is the index of the next pair, an entry <= 0 is minus a leaf (RFC 6386 8.1)
const int8_t kVp8KfYmodeTree[8] = {-VP8_B_PRED, 2, 4, 6, -VP8_DC_PRED, -VP8_V_PRED, -VP8_H_PRED, -VP8_TM_PRED};
const int8_t kVp8UvModeTree[6] = {-VP8_DC_PRED, 2, -VP8_V_PRED, 4, -VP8_H_PRED, -VP8_TM_PRED};
const int8_t kVp8BmodeTree[18] = {-VP8_B_DC, 2, -VP8_B_TM, 4, -VP8_B_VE, 6, 8, 12, -VP8_B_HE, 10, -VP8_B_RD, -VP8_B_VR, -VP8_B_LD, 14, -VP8_B_VL, 16, -VP8_B_HD, -VP8_B_HU};
const int8_t kVp8SegmentTree[6] = {2, 4, -0, -1, -2, -3};
// tokens: 0..4 the values 0..4, 5..10 DCT_CAT1..6, 11 end of block
const int8_t kVp8CoefTree[22] = {-11, 2, -0, 4, -1, 6, 8, 12, -2, 10, -3, -4, 14, 16, -5, -6, 18, 20, -7, -8, -9, -10};
const uint8_t kVp8CoefBands[16] = {0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7};
const uint8_t kVp8Zigzag[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
const uint8_t kVp8CatProbs[6][12] = {{159, 0}, {165, 145, 0}, {173, 148, 140, 0}, {176, 155, 140, 135, 0}, {180, 157, 141, 134, 130, 0},
                                     {254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129, 0}};
const uint8_t kVp8CatBase[6] = {5, 7, 11, 19, 35, 67};

// inter frames: 16.2 (modes of frames that are no key frames), 16.3 (mode and vector contexts), 17.2 (vector probabilities)
const uint8_t kVp8YmodeProb[4] = {112, 86, 140, 37}, kVp8UvModeProb[3] = {162, 101, 204};
const uint8_t kVp8BmodeProb[9] = {120, 90, 79, 133, 87, 85, 80, 111, 151};
const int8_t kVp8YmodeTree[8] = {-VP8_DC_PRED, 2, 4, 6, -VP8_V_PRED, -VP8_H_PRED, -VP8_TM_PRED, -VP8_B_PRED};
// leaves: 0 ZERO, 1 NEAREST, 2 NEAR, 3 NEW, 4 SPLIT (VP8_MV_* - 1)
const int8_t kVp8MvRefTree[8] = {-0, 2, -1, 4, -2, 6, -3, -4};
// leaves: 0 LEFT4x4, 1 ABOVE4x4, 2 ZERO4x4, 3 NEW4x4
const int8_t kVp8SubMvRefTree[6] = {-0, 2, -1, 4, -2, -3};
// leaves: 0 16x8 (top / bottom), 1 8x16 (left / right), 2 quarters, 3 sixteen 4x4
const int8_t kVp8SplitTree[6] = {-3, 2, -2, 4, -0, -1};
const int8_t kVp8SmallMvTree[14] = {2, 8, 4, 6, -0, -1, -2, -3, 10, 12, -4, -5, -6, -7};
const uint8_t kVp8ModeContexts[6][4] = {{7, 1, 1, 143}, {14, 18, 14, 107}, {135, 64, 57, 68}, {60, 56, 128, 65}, {159, 134, 128, 34}, {234, 188, 128, 28}};
// contexts: 0 normal, 1 left is zero, 2 above is zero, 3 left equals above, 4 both zero
const uint8_t kVp8SubMvRefProbs[5][3] = {{147, 136, 18}, {106, 145, 1}, {179, 121, 1}, {223, 1, 34}, {208, 1, 1}};
const uint8_t kVp8SplitProbs[3] = {110, 111, 150};
const uint8_t kVp8MvDefaultProbs[2][19] = {{162, 128, 225, 146, 172, 147, 214, 39, 156, 128, 129, 132, 75, 145, 178, 206, 239, 254, 254},
                                           {164, 128, 204, 170, 119, 235, 140, 230, 228, 128, 130, 130, 74, 148, 180, 203, 236, 254, 254}};
const uint8_t kVp8MvUpdateProbs[2][19] = {{237, 246, 253, 253, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 250, 250, 252, 254, 254},
                                          {231, 243, 245, 253, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 251, 251, 254, 254, 254}};
const uint8_t kVp8Splits[4][16] = {{0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1}, {0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1},
                                   {0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}};

const uint8_t kVp8KfBmodeProbs[10][10][9] = {
    {{231, 120, 48, 89, 115, 113, 120, 152, 112}, {152, 179, 64, 126, 170, 118, 46, 70, 95}, {175, 69, 143, 80, 85, 82, 72, 155, 103},
     {56, 58, 10, 171, 218, 189, 17, 13, 152}, {144, 71, 10, 38, 171, 213, 144, 34, 26}, {114, 26, 17, 163, 44, 195, 21, 10, 173},
     {121, 24, 80, 195, 26, 62, 44, 64, 85}, {170, 46, 55, 19, 136, 160, 33, 206, 71}, {63, 20, 8, 114, 114, 208, 12, 9, 226},
     {81, 40, 11, 96, 182, 84, 29, 16, 36}},
    {{134, 183, 89, 137, 98, 101, 106, 165, 148}, {72, 187, 100, 130, 157, 111, 32, 75, 80}, {66, 102, 167, 99, 74, 62, 40, 234, 128},
     {41, 53, 9, 178, 241, 141, 26, 8, 107}, {104, 79, 12, 27, 217, 255, 87, 17, 7}, {74, 43, 26, 146, 73, 166, 49, 23, 157},
     {65, 38, 105, 160, 51, 52, 31, 115, 128}, {87, 68, 71, 44, 114, 51, 15, 186, 23}, {47, 41, 14, 110, 182, 183, 21, 17, 194},
     {66, 45, 25, 102, 197, 189, 23, 18, 22}},
    {{88, 88, 147, 150, 42, 46, 45, 196, 205}, {43, 97, 183, 117, 85, 38, 35, 179, 61}, {39, 53, 200, 87, 26, 21, 43, 232, 171},
     {56, 34, 51, 104, 114, 102, 29, 93, 77}, {107, 54, 32, 26, 51, 1, 81, 43, 31}, {39, 28, 85, 171, 58, 165, 90, 98, 64},
     {34, 22, 116, 206, 23, 34, 43, 166, 73}, {68, 25, 106, 22, 64, 171, 36, 225, 114}, {34, 19, 21, 102, 132, 188, 16, 76, 124},
     {62, 18, 78, 95, 85, 57, 50, 48, 51}},
    {{193, 101, 35, 159, 215, 111, 89, 46, 111}, {60, 148, 31, 172, 219, 228, 21, 18, 111}, {112, 113, 77, 85, 179, 255, 38, 120, 114},
     {40, 42, 1, 196, 245, 209, 10, 25, 109}, {100, 80, 8, 43, 154, 1, 51, 26, 71}, {88, 43, 29, 140, 166, 213, 37, 43, 154},
     {61, 63, 30, 155, 67, 45, 68, 1, 209}, {142, 78, 78, 16, 255, 128, 34, 197, 171}, {41, 40, 5, 102, 211, 183, 4, 1, 221},
     {51, 50, 17, 168, 209, 192, 23, 25, 82}},
    {{125, 98, 42, 88, 104, 85, 117, 175, 82}, {95, 84, 53, 89, 128, 100, 113, 101, 45}, {75, 79, 123, 47, 51, 128, 81, 171, 1},
     {57, 17, 5, 71, 102, 57, 53, 41, 49}, {115, 21, 2, 10, 102, 255, 166, 23, 6}, {38, 33, 13, 121, 57, 73, 26, 1, 85},
     {41, 10, 67, 138, 77, 110, 90, 47, 114}, {101, 29, 16, 10, 85, 128, 101, 196, 26}, {57, 18, 10, 102, 102, 213, 34, 20, 43},
     {117, 20, 15, 36, 163, 128, 68, 1, 26}},
    {{138, 31, 36, 171, 27, 166, 38, 44, 229}, {67, 87, 58, 169, 82, 115, 26, 59, 179}, {63, 59, 90, 180, 59, 166, 93, 73, 154},
     {40, 40, 21, 116, 143, 209, 34, 39, 175}, {57, 46, 22, 24, 128, 1, 54, 17, 37}, {47, 15, 16, 183, 34, 223, 49, 45, 183},
     {46, 17, 33, 183, 6, 98, 15, 32, 183}, {65, 32, 73, 115, 28, 128, 23, 128, 205}, {40, 3, 9, 115, 51, 192, 18, 6, 223},
     {87, 37, 9, 115, 59, 77, 64, 21, 47}},
    {{104, 55, 44, 218, 9, 54, 53, 130, 226}, {64, 90, 70, 205, 40, 41, 23, 26, 57}, {54, 57, 112, 184, 5, 41, 38, 166, 213},
     {30, 34, 26, 133, 152, 116, 10, 32, 134}, {75, 32, 12, 51, 192, 255, 160, 43, 51}, {39, 19, 53, 221, 26, 114, 32, 73, 255},
     {31, 9, 65, 234, 2, 15, 1, 118, 73}, {88, 31, 35, 67, 102, 85, 55, 186, 85}, {56, 21, 23, 111, 59, 205, 45, 37, 192},
     {55, 38, 70, 124, 73, 102, 1, 34, 98}},
    {{102, 61, 71, 37, 34, 53, 31, 243, 192}, {69, 60, 71, 38, 73, 119, 28, 222, 37}, {68, 45, 128, 34, 1, 47, 11, 245, 171},
     {62, 17, 19, 70, 146, 85, 55, 62, 70}, {75, 15, 9, 9, 64, 255, 184, 119, 16}, {37, 43, 37, 154, 100, 163, 85, 160, 1},
     {63, 9, 92, 136, 28, 64, 32, 201, 85}, {86, 6, 28, 5, 64, 255, 25, 248, 1}, {56, 8, 17, 132, 137, 255, 55, 116, 128},
     {58, 15, 20, 82, 135, 57, 26, 121, 40}},
    {{164, 50, 31, 137, 154, 133, 25, 35, 218}, {51, 103, 44, 131, 131, 123, 31, 6, 158}, {86, 40, 64, 135, 148, 224, 45, 183, 128},
     {22, 26, 17, 131, 240, 154, 14, 1, 209}, {83, 12, 13, 54, 192, 255, 68, 47, 28}, {45, 16, 21, 91, 64, 222, 7, 1, 197},
     {56, 21, 39, 155, 60, 138, 23, 102, 213}, {85, 26, 85, 85, 128, 128, 32, 146, 171}, {18, 11, 7, 63, 144, 171, 4, 4, 246},
     {35, 27, 10, 146, 174, 171, 12, 26, 128}},
    {{190, 80, 35, 99, 180, 80, 126, 54, 45}, {85, 126, 47, 87, 176, 51, 41, 20, 32}, {101, 75, 128, 139, 118, 146, 116, 128, 85},
     {56, 41, 15, 176, 236, 85, 37, 9, 62}, {146, 36, 19, 30, 171, 255, 97, 27, 20}, {71, 30, 17, 119, 118, 255, 17, 18, 138},
     {101, 38, 60, 138, 55, 70, 43, 26, 142}, {138, 45, 61, 62, 219, 1, 81, 188, 64}, {32, 41, 20, 117, 151, 142, 20, 21, 163},
     {112, 19, 12, 61, 195, 128, 48, 4, 24}},
};

// ---- frame tag ------------------------------------------------------------------------------------------------------------------------------------
std::string vp8_read_tag(const uint8_t *p, size_t n, bool first, Vp8FrameTag &tag, bool inter_ok) {
    uint8_t b[10] = {0};
    memcpy(b, p, n < 10 ? n : 10);                       // (a frame shorter than its header reads zeros, like a partition that ends early)
    const uint32_t t = b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16;
    tag.key = !(t & 1); tag.version = (int)(t >> 1 & 7); tag.show = (int)(t >> 4 & 1); tag.part1 = t >> 5;
    if (!tag.key && (first || !inter_ok)) return first ? "VP8: the first frame is not a key frame" : "VP8 inter frames are not built";
    if (tag.version > 3) { char m[96]; snprintf(m, sizeof m, "VP8: version %d is not defined (RFC 6386 9.1)", tag.version); return m; }
    if (!tag.key) return "";                             // (an inter frame has no start code and no size: it keeps the key frame's)
    if (b[3] != 0x9d || b[4] != 0x01 || b[5] != 0x2a) return "VP8: bad start code";
    tag.width = (b[6] | b[7] << 8) & 0x3fff; tag.hscale = b[7] >> 6;
    tag.height = (b[8] | b[9] << 8) & 0x3fff; tag.vscale = b[9] >> 6;
    if (tag.width == 0 || tag.height == 0 || tag.width > kVp8MaxDim || tag.height > kVp8MaxDim) {
        char m[96]; snprintf(m, sizeof m, "VP8: picture size %dx%d is not supported", tag.width, tag.height); return m;
    }
    return "";
}

// ---- one frame ------------------------------------------------------------------------------------------------------------------------------------
namespace {

inline int clampq(int i) { return i < 0 ? 0 : (i > 127 ? 127 : i); }

// the tokens of one block (RFC 6386 13.2, 13.3): entries for its non-zero levels; returns 1 when a token other than end-of-block was read
inline int vp8_block_tokens(Vp8Bool &d, const uint8_t probs[8][3][11], int ctx, int first, int blk, std::vector<uint32_t> &entries) {
    int i = first, start = 0;
    while (i < 16) {
        const int t = d.tree(kVp8CoefTree, probs[kVp8CoefBands[i]][ctx], start);
        if (t == 11) break;
        if (t == 0) { ctx = 0; start = 2; i++; continue; }       // (no end-of-block can follow a zero: the tree is entered past its first branch)
        int v = t;
        if (t > 4) {
            const uint8_t *cp = kVp8CatProbs[t - 5];
            int extra = 0;
            while (*cp) extra = extra << 1 | d.read(*cp++);
            v = kVp8CatBase[t - 5] + extra;
        }
        ctx = v == 1 ? 1 : 2;
        if (d.read(128)) v = -v;
        entries.push_back((uint32_t)kVp8Zigzag[i] | (uint32_t)blk << 4 | (uint32_t)(uint16_t)(int16_t)v << 16);
        start = 0; i++;
    }
    return i > first ? 1 : 0;
}

// ---- inter frames: vectors (RFC 6386 16.3, 17) ----
struct Mv { int16_t r = 0, c = 0; bool zero() const { return !r && !c; } bool operator==(const Mv &o) const { return r == o.r && c == o.c; } };
// what the near-vector search and the split contexts read of a macroblock; everything outside the frame is an intra macroblock with zero vectors
struct MbMv { uint8_t ref = 0, split = 0; Mv mv; Mv b[16]; };

// 17.2: one component, in quarter samples; the caller doubles it
inline int vp8_read_mv_comp(Vp8Bool &d, const uint8_t *p) {
    int x = 0;
    if (d.read(p[0])) {                                   // the long form: bits 0, 1, 2, then 9 down to 4, then bit 3 -- which is read only when some
        for (int i = 0; i < 3; i++) x += d.read(p[9 + i]) << i;       // higher bit is set: a long vector of less than 8 would have been a short one
        for (int i = 9; i > 3; i--) x += d.read(p[9 + i]) << i;
        if (!(x & 0xfff0) || d.read(p[9 + 3])) x += 8;
    } else x = d.tree(kVp8SmallMvTree, p + 2);
    if (x && d.read(p[1])) x = -x;
    return x;
}
inline Mv vp8_read_mv(Vp8Bool &d, const uint8_t mvp[2][19], Mv base) {
    Mv m;
    const int r = vp8_read_mv_comp(d, mvp[0]) * 2, c = vp8_read_mv_comp(d, mvp[1]) * 2;
    m.r = (int16_t)(base.r + r); m.c = (int16_t)(base.c + c);      // (16-bit sums: whatever a damaged stream adds up wraps, on the device as here)
    return m;
}
inline int16_t clamp_i16(int v, int lo, int hi) { return (int16_t)(v < lo ? lo : (v > hi ? hi : v)); }

}  // namespace

void Vp8State::reset_key(int w, int h) {
    memcpy(e.coef, kVp8CoefProbs, sizeof e.coef); memcpy(e.mv, kVp8MvDefaultProbs, sizeof e.mv);
    memcpy(e.ymode, kVp8YmodeProb, sizeof e.ymode); memcpy(e.uvmode, kVp8UvModeProb, sizeof e.uvmode);
    seg_abs = 0;
    for (int i = 0; i < 4; i++) seg_q[i] = seg_lf[i] = ref_delta[i] = mode_delta[i] = sign_bias[i] = 0;
    mb_w = w; mb_h = h;
    seg_map.assign((size_t)w * h, 0);
}

void vp8_decode_frame(const uint8_t *p, size_t n, Vp8Pic &pic, Vp8State *st) {
    const Vp8FrameTag &tag = pic.tag;
    const bool key = tag.key || !st;           // (without a state there are only key frames: vp8_read_tag refused the others)
    const size_t hdr = key ? 10 : 3;
    pic.damaged = n < hdr;
    const uint8_t *body = n > hdr ? p + hdr : p + n;
    const size_t body_n = n > hdr ? n - hdr : 0;
    size_t part1 = tag.part1;
    if (part1 > body_n) { part1 = body_n; pic.damaged = true; }
    const int mb_w = (tag.width + 15) >> 4, mb_h = (tag.height + 15) >> 4;
    // what the frames before left behind: nothing for a key frame (9.3, 9.6, 9.7: segmentation, the loop filter deltas, the sign biases and every
    // probability start from their defaults), and nothing either for an inter frame whose state is of another size (a caller's mistake, kept harmless)
    Vp8State local;
    Vp8State &S = st ? *st : local;
    if (key || S.mb_w != mb_w || S.mb_h != mb_h || S.seg_map.size() != (size_t)mb_w * mb_h) S.reset_key(mb_w, mb_h);
    Vp8Bool d; d.init(body, part1);
    pic.color_space = pic.clamping = 0;
    if (key) { pic.color_space = d.literal(1); pic.clamping = d.literal(1); }
    // segmentation (9.3): the data and the map persist until a frame updates them
    int (&seg_q)[4] = S.seg_q, (&seg_lf)[4] = S.seg_lf; uint8_t seg_probs[3] = {255, 255, 255};
    pic.update_map = 0;
    pic.seg_on = d.literal(1);
    if (pic.seg_on) {
        pic.update_map = d.literal(1);
        if (d.literal(1)) {
            S.seg_abs = d.literal(1);
            for (int &q : seg_q) q = d.flagged(7);
            for (int &l : seg_lf) l = d.flagged(6);
        }
        if (pic.update_map) for (uint8_t &pr : seg_probs) pr = d.literal(1) ? (uint8_t)d.literal(8) : 255;
    }
    pic.seg_abs = S.seg_abs;
    pic.filter_type = d.literal(1); pic.level = d.literal(6); pic.sharpness = d.literal(3);
    // the loop filter deltas (9.6): a delta whose flag is clear keeps its value
    int (&ref_delta)[4] = S.ref_delta, (&mode_delta)[4] = S.mode_delta;
    pic.delta_on = d.literal(1);
    if (pic.delta_on && d.literal(1)) {
        for (int &v : ref_delta) if (d.literal(1)) { v = d.literal(6); if (d.literal(1)) v = -v; }
        for (int &v : mode_delta) if (d.literal(1)) { v = d.literal(6); if (d.literal(1)) v = -v; }
    }
    pic.n_parts = 1 << d.literal(2);
    const int yac = d.literal(7);
    const int ydc = d.flagged(4), y2dc = d.flagged(4), y2ac = d.flagged(4), uvdc = d.flagged(4), uvac = d.flagged(4);
    pic.refresh_golden = pic.refresh_alt = pic.copy_to_golden = pic.copy_to_alt = 0; pic.refresh_last = 1;
    if (!key) {                                // 9.7: which references this frame becomes, and which take over another's picture
        pic.refresh_golden = d.literal(1); pic.refresh_alt = d.literal(1);
        if (!pic.refresh_golden) pic.copy_to_golden = d.literal(2);
        if (!pic.refresh_alt) pic.copy_to_alt = d.literal(2);
        S.sign_bias[2] = d.literal(1); S.sign_bias[3] = d.literal(1);
    }
    // 9.11: refresh_entropy_probs 0 -- what this frame changes of the probabilities is dropped when the frame is done
    pic.refresh_entropy = d.literal(1);
    Vp8Entropy saved;
    if (!pic.refresh_entropy) saved = S.e;
    if (!key) pic.refresh_last = d.literal(1);
    uint8_t (&probs)[4][8][3][11] = S.e.coef;
    pic.prob_updates = 0;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 8; j++) for (int k = 0; k < 3; k++) for (int l = 0; l < 11; l++)
        if (d.read(kVp8CoefUpdateProbs[i][j][k][l])) { probs[i][j][k][l] = (uint8_t)d.literal(8); pic.prob_updates++; }
    pic.no_coeff_skip = d.literal(1);
    const int prob_skip = pic.no_coeff_skip ? d.literal(8) : 0;
    pic.prob_intra = pic.prob_last = pic.prob_gf = pic.mode_prob_updates = pic.mv_prob_updates = 0;
    if (!key) {                                // 9.10, 16.2, 17.2
        pic.prob_intra = d.literal(8); pic.prob_last = d.literal(8); pic.prob_gf = d.literal(8);
        if (d.literal(1)) { for (uint8_t &v : S.e.ymode) v = (uint8_t)d.literal(8); pic.mode_prob_updates++; }
        if (d.literal(1)) { for (uint8_t &v : S.e.uvmode) v = (uint8_t)d.literal(8); pic.mode_prob_updates++; }
        for (int i = 0; i < 2; i++) for (int j = 0; j < 19; j++)
            if (d.read(kVp8MvUpdateProbs[i][j])) { const int x = d.literal(7); S.e.mv[i][j] = (uint8_t)(x ? x << 1 : 1); pic.mv_prob_updates++; }
    }
    // 9.6, 14.1: the dequantisation factors per segment
    for (int s = 0; s < 4; s++) {
        int base = yac;
        if (pic.seg_on) base = pic.seg_abs ? seg_q[s] : yac + seg_q[s];
        base = clampq(base);
        pic.dq[s][0] = (int16_t)kVp8DcQ[clampq(base + ydc)]; pic.dq[s][1] = (int16_t)kVp8AcQ[base];
        pic.dq[s][2] = (int16_t)(kVp8DcQ[clampq(base + y2dc)] * 2);
        pic.dq[s][3] = (int16_t)std::max(kVp8AcQ[clampq(base + y2ac)] * 155 / 100, 8);
        pic.dq[s][4] = (int16_t)std::min<int>(kVp8DcQ[clampq(base + uvdc)], 132); pic.dq[s][5] = (int16_t)kVp8AcQ[clampq(base + uvac)];
    }
    // 9.5: the token partitions
    const uint8_t *rest = body + part1; size_t rest_n = body_n - part1;
    const size_t sizes_len = 3 * (size_t)(pic.n_parts - 1);
    uint8_t sizes[21] = {0};
    memcpy(sizes, rest, std::min(sizes_len, rest_n));
    if (rest_n < sizes_len) { pic.damaged = true; rest += rest_n; rest_n = 0; } else { rest += sizes_len; rest_n -= sizes_len; }
    Vp8Bool parts[8];
    size_t o = 0;
    for (int k = 0; k < pic.n_parts; k++) {
        size_t len = k < pic.n_parts - 1 ? (size_t)sizes[3 * k] | (size_t)sizes[3 * k + 1] << 8 | (size_t)sizes[3 * k + 2] << 16 : rest_n - std::min(o, rest_n);
        const size_t at = std::min(o, rest_n);
        if (len > rest_n - at) { pic.damaged = true; len = rest_n - at; }
        parts[k].init(rest + at, len);
        o = at + len;
    }
    pic.mb_w = mb_w; pic.mb_h = mb_h;
    pic.mbs.assign((size_t)mb_w * mb_h, Vp8Mb());
    pic.entries.clear(); pic.split.clear();
    pic.bpred_mbs = pic.skipped_mbs = 0; pic.segments_used = 0; pic.filtered = false;
    pic.inter_mbs = pic.golden_mbs = pic.alt_mbs = pic.split_mbs = pic.intra_mbs = 0;
    // inter frames: the vectors of the frame's macroblocks inside a border of "intra, zero vector" (16.3: so counts everything outside the frame)
    const int ms = mb_w + 1;
    static thread_local std::vector<MbMv> mvs;
    if (!key) mvs.assign((size_t)ms * (mb_h + 1), MbMv());
    // contexts: sub-block modes of the macroblocks above (their bottom row), non-zero flags above (4 Y, 2 U, 2 V, 1 Y2 per column)
    std::vector<uint8_t> above_b((size_t)mb_w * 4, VP8_B_DC), above_nz((size_t)mb_w * 9, 0);
    static const uint8_t implied[4] = {VP8_B_DC, VP8_B_VE, VP8_B_HE, VP8_B_TM};
    for (int my = 0; my < mb_h; my++) {
        uint8_t left_b[4] = {VP8_B_DC, VP8_B_DC, VP8_B_DC, VP8_B_DC}, ln[9] = {0};
        Vp8Bool &tok = parts[my % pic.n_parts];                 // macroblock row r reads partition r mod n
        for (int mx = 0; mx < mb_w; mx++) {
            Vp8Mb &m = pic.mbs[(size_t)my * mb_w + mx];
            memset(&m, 0, sizeof m);
            uint8_t &seg = S.seg_map[(size_t)my * mb_w + mx];
            if (pic.update_map) seg = (uint8_t)d.tree(kVp8SegmentTree, seg_probs);
            m.segment = seg;                    // (a frame that does not update the map keeps the one it found: all zero behind a key frame)
            const int skip = pic.no_coeff_skip ? d.read(prob_skip) : 0;
            int ref = 0;                        // 0 intra, 1 last, 2 golden, 3 altref
            uint8_t *ab = &above_b[(size_t)mx * 4];
            if (!key && d.read(pic.prob_intra)) {
                // ---- an inter macroblock (16.3) ----
                ref = 1;
                if (d.read(pic.prob_last)) ref = 2 + d.read(pic.prob_gf);
                const MbMv &A = mvs[(size_t)my * ms + mx + 1], &L = mvs[(size_t)(my + 1) * ms + mx], &AL = mvs[(size_t)my * ms + mx];
                MbMv &cur = mvs[(size_t)(my + 1) * ms + mx + 1];
                // the near-vector search: above and left weigh 2, above-left 1; a neighbour whose reference has the other sign bias counts inverted
                Mv near[4]; int cnt[4] = {0, 0, 0, 0}, k = 0;
                const MbMv *nb[3] = {&A, &L, &AL};
                for (int q = 0; q < 3; q++) {
                    const MbMv &o = *nb[q];
                    if (!o.ref) continue;
                    if (!o.mv.zero()) {
                        Mv t = o.mv;
                        if (S.sign_bias[o.ref] != S.sign_bias[ref]) { t.r = (int16_t)-t.r; t.c = (int16_t)-t.c; }
                        if (q == 0 || !(t == near[k])) near[++k] = t;
                        cnt[k] += q < 2 ? 2 : 1;
                    } else cnt[0] += q < 2 ? 2 : 1;
                }
                if (cnt[3] && near[k] == near[1]) cnt[1] += 1;        // three distinct vectors found, and the last equals the first
                cnt[3] = ((A.split ? 1 : 0) + (L.split ? 1 : 0)) * 2 + (AL.split ? 1 : 0);
                if (cnt[2] > cnt[1]) { std::swap(cnt[1], cnt[2]); std::swap(near[1], near[2]); }
                if (cnt[1] >= cnt[0]) near[0] = near[1];
                // best, nearest and near are clamped to the window a macroblock beyond the frame's edges (16.3; the vectors that are read are not)
                const int lo_c = -(mx * 128) - 128, hi_c = (mb_w - 1 - mx) * 128 + 128, lo_r = -(my * 128) - 128, hi_r = (mb_h - 1 - my) * 128 + 128;
                for (int q = 0; q < 3; q++) { near[q].r = clamp_i16(near[q].r, lo_r, hi_r); near[q].c = clamp_i16(near[q].c, lo_c, hi_c); }
                uint8_t mp[4];
                for (int q = 0; q < 4; q++) mp[q] = kVp8ModeContexts[cnt[q]][q];
                const int mode = d.tree(kVp8MvRefTree, mp);
                m.mvmode = (uint8_t)(mode + 1);
                Vp8InterInfo ii; memset(&ii, 0, sizeof ii);
                ii.ref = (uint8_t)ref;
                cur.ref = (uint8_t)ref;
                if (mode == 4) {
                    const int kind = d.tree(kVp8SplitTree, kVp8SplitProbs);
                    static const int n_parts_of[4] = {2, 2, 4, 16};
                    for (int j = 0; j < n_parts_of[kind]; j++) {
                        int b0 = 0;
                        while (kVp8Splits[kind][b0] != j) b0++;
                        const Mv lm = (b0 & 3) ? cur.b[b0 - 1] : L.b[b0 + 3], am = (b0 >> 2) ? cur.b[b0 - 4] : A.b[b0 + 12];
                        const int ctx = lm == am ? (lm.zero() ? 4 : 3) : (am.zero() ? 2 : (lm.zero() ? 1 : 0));
                        const int sub = d.tree(kVp8SubMvRefTree, kVp8SubMvRefProbs[ctx]);
                        const Mv v = sub == 0 ? lm : (sub == 1 ? am : (sub == 2 ? Mv() : vp8_read_mv(d, S.e.mv, near[0])));
                        for (int b = 0; b < 16; b++) if (kVp8Splits[kind][b] == j) cur.b[b] = v;
                    }
                    cur.mv = cur.b[15]; cur.split = 1;
                    ii.split = (uint8_t)(1 + kind); ii.split_idx = (uint32_t)pic.split.size();
                    Vp8SplitMv sv;
                    for (int b = 0; b < 16; b++) { sv.y[b][0] = cur.b[b].c; sv.y[b][1] = cur.b[b].r; }
                    for (int g = 0; g < 4; g++) {
                        const int b = (g >> 1) * 8 + (g & 1) * 2;
                        int sc = cur.b[b].c + cur.b[b + 1].c + cur.b[b + 4].c + cur.b[b + 5].c, sr = cur.b[b].r + cur.b[b + 1].r + cur.b[b + 4].r + cur.b[b + 5].r;
                        sc = (sc < 0 ? sc - 4 : sc + 4) / 8; sr = (sr < 0 ? sr - 4 : sr + 4) / 8;       // (the sum of four, rounded away from zero)
                        if (tag.version == 3) { sc &= ~7; sr &= ~7; }
                        sv.c[g][0] = (int16_t)sc; sv.c[g][1] = (int16_t)sr;
                    }
                    pic.split.push_back(sv);
                    pic.split_mbs++;
                    m.ymode = VP8_B_PRED;       // (no Y2 block, inner edges always filtered: what the device and the token loop below read of it)
                } else {
                    cur.mv = mode == 0 ? Mv() : (mode == 1 ? near[1] : (mode == 2 ? near[2] : vp8_read_mv(d, S.e.mv, near[0])));
                    for (Mv &b : cur.b) b = cur.mv;
                    m.ymode = VP8_DC_PRED;
                }
                ii.mvx = cur.mv.c; ii.mvy = cur.mv.r;
                int cc = (cur.mv.c + (cur.mv.c < 0 ? -1 : 1)) / 2, cr = (cur.mv.r + (cur.mv.r < 0 ? -1 : 1)) / 2;
                if (tag.version == 3) { cc &= ~7; cr &= ~7; }
                ii.cmvx = (int16_t)cc; ii.cmvy = (int16_t)cr;
                memcpy(m.bmodes, &ii, sizeof ii);
                m.flags |= VP8_MB_INTER;
                pic.inter_mbs++; if (ref == 2) pic.golden_mbs++; if (ref == 3) pic.alt_mbs++;
                memset(ab, VP8_B_DC, 4); memset(left_b, VP8_B_DC, 4);
            } else {
                m.ymode = key ? (uint8_t)d.tree(kVp8KfYmodeTree, kVp8KfYmodeProb) : (uint8_t)d.tree(kVp8YmodeTree, S.e.ymode);
                if (m.ymode == VP8_B_PRED) {
                    for (int b = 0; b < 16; b++) {
                        const int A = b < 4 ? ab[b & 3] : m.bmodes[b - 4], L = (b & 3) ? m.bmodes[b - 1] : left_b[b >> 2];
                        // (16.2: outside key frames the sub-block modes are coded without contexts)
                        m.bmodes[b] = (uint8_t)d.tree(kVp8BmodeTree, key ? kVp8KfBmodeProbs[A][L] : kVp8BmodeProb);
                    }
                    pic.bpred_mbs++;
                } else memset(m.bmodes, implied[m.ymode], 16);
                for (int k = 0; k < 4; k++) { ab[k] = m.bmodes[12 + k]; left_b[k] = m.bmodes[4 * k + 3]; }
                m.uvmode = (uint8_t)d.tree(kVp8UvModeTree, key ? kVp8KfUvModeProb : S.e.uvmode);
                pic.intra_mbs++;
            }
            if (pic.seg_on) pic.segments_used |= 1 << m.segment;
            // residual data (13)
            uint8_t *an = &above_nz[(size_t)mx * 9];
            m.first = (uint32_t)pic.entries.size();
            bool any = false;
            if (skip) {
                pic.skipped_mbs++;
                const uint8_t ka = an[8], kl = ln[8];
                memset(an, 0, 9); memset(ln, 0, 9);
                if (m.ymode == VP8_B_PRED) { an[8] = ka; ln[8] = kl; }     // (no Y2 block: its context stays)
            } else {
                int first = 0;
                auto block = [&](const uint8_t pr[8][3][11], uint8_t &a, uint8_t &l, int fst, int blk) {
                    const size_t before = pic.entries.size();
                    const int nz = vp8_block_tokens(tok, pr, a + l, fst, blk, pic.entries);
                    a = l = (uint8_t)nz; any |= nz != 0;
                    if (pic.entries.size() > before) m.nz |= 1u << blk;
                };
                if (m.ymode != VP8_B_PRED) { block(probs[1], an[8], ln[8], 0, 24); first = 1; }
                for (int b = 0; b < 16; b++) block(probs[first ? 0 : 3], an[b & 3], ln[b >> 2], first, b);
                for (int c = 0; c < 2; c++) for (int b = 0; b < 4; b++) block(probs[2], an[4 + 2 * c + (b & 1)], ln[4 + 2 * c + (b >> 1)], 0, 16 + 4 * c + b);
            }
            m.count = (uint16_t)(pic.entries.size() - m.first);
            if (m.ymode == VP8_B_PRED || any) m.flags |= VP8_MB_INNER;
            // the filter level (9.3, 9.6, 15.1: on a key frame only the intra-frame and the B_PRED deltas can apply)
            int lv = pic.level;
            if (pic.seg_on) lv = pic.seg_abs ? seg_lf[m.segment] : pic.level + seg_lf[m.segment];
            lv = std::min(std::max(lv, 0), 63);
            // (inter frames, 9.6 and the decoder's filter set-up: the delta of the reference, then that of the mode class -- B_PRED for intra
            //  macroblocks, ZERO, SPLIT or "another vector mode" for inter ones)
            if (pic.delta_on) {
                lv += ref_delta[ref];
                if (!ref) { if (m.ymode == VP8_B_PRED) lv += mode_delta[0]; }
                else lv += mode_delta[m.mvmode == VP8_MV_ZERO ? 1 : (m.mvmode == VP8_MV_SPLIT ? 3 : 2)];
                lv = std::min(std::max(lv, 0), 63);
            }
            m.level = (uint8_t)lv;
            pic.filtered |= lv != 0;
        }
    }
    long long past = d.past;
    for (int k = 0; k < pic.n_parts; k++) past = std::max(past, parts[k].past);
    // a bool decoder holds two bytes beyond what it has consumed: up to two zeros past the end are not damage (INTEGRATION.md "VP8")
    if (past > 2) pic.damaged = true;
    if (!pic.refresh_entropy) S.e = saved;
}

std::string vp8_validate_jobs(const Vp8Pic &pic) {
    if (pic.mb_w <= 0 || pic.mb_h <= 0 || pic.mbs.size() != (size_t)pic.mb_w * pic.mb_h) return "VP8 job list: macroblock count";
    for (const Vp8Mb &m : pic.mbs) {
        if (m.ymode > VP8_B_PRED || m.uvmode > VP8_TM_PRED || m.segment > 3 || m.level > 63) return "VP8 job list: a mode, segment or level is out of range";
        if (m.flags & VP8_MB_INTER) {
            Vp8InterInfo ii; memcpy(&ii, m.bmodes, sizeof ii);
            if (pic.tag.key || ii.ref < 1 || ii.ref > 3 || ii.split > 4 || (ii.split != 0) != (m.mvmode == VP8_MV_SPLIT) || m.mvmode < VP8_MV_ZERO || m.mvmode > VP8_MV_SPLIT ||
                (ii.split && ii.split_idx >= pic.split.size()) || (m.ymode != VP8_DC_PRED && m.ymode != VP8_B_PRED) || (m.ymode == VP8_B_PRED) != (ii.split != 0))
                return "VP8 job list: an inter macroblock's reference, mode or vector index is out of range";
        } else {
            if (m.mvmode) return "VP8 job list: an intra macroblock with a vector mode";
            for (uint8_t b : m.bmodes) if (b > VP8_B_HU) return "VP8 job list: a sub-block mode is out of range";
        }
        if (m.count > kVp8MaxMbEntries || (size_t)m.first + m.count > pic.entries.size()) return "VP8 job list: a macroblock's entries lie outside the list";
        for (uint32_t e = 0; e < m.count; e++) {
            const uint32_t v = pic.entries[m.first + e]; const int blk = (int)(v >> 4 & 31);
            if (blk > 24 || (blk == 24 && m.ymode == VP8_B_PRED) || (v & 0xfe00)) return "VP8 job list: an entry names a block the macroblock does not have";
        }
    }
    return "";
}

}  // namespace jmamd
