"""RFC 6386 key-frame decoding restated in numpy / plain Python (test reference for codec_type 5, option vp8).

Written from the RFC's text and its decoding procedures, with tables typed in here; nothing is shared with jmcodec_amd/csrc/vp8_syntax.cpp.
What it decodes, refuses and how it treats damage is the library's contract (INTEGRATION.md "VP8"):
  * input: an IVF byte stream ("DKIF") or a list of frames; RIFF / WebP wrappers are stripped by webp_payload();
  * every key frame of the RFC; an inter frame, a first frame that is no key frame, a bad start code and an oversized picture raise Refused;
  * a bool decoder that runs past the end of its partition reads zeros (RFC 7.3); a picture in which one read more than two bytes past the end, or
    whose partitions overrun the frame, counts in `errors` and still decodes, deterministically.
Where the RFC leaves an edge open, libwebp decides (tests/golden/vp8): the above-right samples of the last macroblock of a row below the first repeat
sample 15 of the row above the macroblock; the corner sample is 127 in the first macroblock row and 129 in the first column below it.
"""
import struct

import numpy as np

from jpeg_ref import frame_bytes

MAX_DIM = 8192      # (the MJPEG path's limit)


class Refused(Exception):
    pass


# ---- tables (RFC 6386 sections 14.1, 13.4, 13.5, 11.2-11.5, 13.2) ----
DC_Q = [
    4, 5, 6, 7, 8, 9, 10, 10, 11, 12, 13, 14, 15, 16, 17, 17, 18, 19, 20, 20, 21, 21, 22, 22, 23, 23, 24, 25, 25, 26, 27, 28,
    29, 30, 31, 32, 33, 34, 35, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58,
    59, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 76, 77, 78, 79, 80, 81, 82, 83, 84, 85, 86, 87, 88, 89,
    91, 93, 95, 96, 98, 100, 101, 102, 104, 106, 108, 110, 112, 114, 116, 118, 122, 124, 126, 128, 130, 132, 134, 136, 138, 140, 143, 145, 148, 151, 154, 157]
AC_Q = [
    4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35,
    36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 60, 62, 64, 66, 68, 70, 72, 74, 76,
    78, 80, 82, 84, 86, 88, 90, 92, 94, 96, 98, 100, 102, 104, 106, 108, 110, 112, 114, 116, 119, 122, 125, 128, 131, 134, 137, 140, 143, 146, 149, 152,
    155, 158, 161, 164, 167, 170, 173, 177, 181, 185, 189, 193, 197, 201, 205, 209, 213, 217, 221, 225, 229, 234, 239, 245, 249, 254, 259, 264, 269, 274, 279, 284]

_ = 128
DEFAULT_COEF_PROBS = [
    [   # block type 0: Y after Y2
        [[_] * 11, [_] * 11, [_] * 11],
        [[253, 136, 254, 255, 228, 219, _, _, _, _, _], [189, 129, 242, 255, 227, 213, 255, 219, _, _, _], [106, 126, 227, 252, 214, 209, 255, 255, _, _, _]],
        [[1, 98, 248, 255, 236, 226, 255, 255, _, _, _], [181, 133, 238, 254, 221, 234, 255, 154, _, _, _], [78, 134, 202, 247, 198, 180, 255, 219, _, _, _]],
        [[1, 185, 249, 255, 243, 255, _, _, _, _, _], [184, 150, 247, 255, 236, 224, _, _, _, _, _], [77, 110, 216, 255, 236, 230, _, _, _, _, _]],
        [[1, 101, 251, 255, 241, 255, _, _, _, _, _], [170, 139, 241, 252, 236, 209, 255, 255, _, _, _], [37, 116, 196, 243, 228, 255, 255, 255, _, _, _]],
        [[1, 204, 254, 255, 245, 255, _, _, _, _, _], [207, 160, 250, 255, 238, _, _, _, _, _, _], [102, 103, 231, 255, 211, 171, _, _, _, _, _]],
        [[1, 152, 252, 255, 240, 255, _, _, _, _, _], [177, 135, 243, 255, 234, 225, _, _, _, _, _], [80, 129, 211, 255, 194, 224, _, _, _, _, _]],
        [[1, 1, 255, _, _, _, _, _, _, _, _], [246, 1, 255, _, _, _, _, _, _, _, _], [255, _, _, _, _, _, _, _, _, _, _]],
    ],
    [   # block type 1: Y2
        [[198, 35, 237, 223, 193, 187, 162, 160, 145, 155, 62], [131, 45, 198, 221, 172, 176, 220, 157, 252, 221, 1], [68, 47, 146, 208, 149, 167, 221, 162, 255, 223, _]],
        [[1, 149, 241, 255, 221, 224, 255, 255, _, _, _], [184, 141, 234, 253, 222, 220, 255, 199, _, _, _], [81, 99, 181, 242, 176, 190, 249, 202, 255, 255, _]],
        [[1, 129, 232, 253, 214, 197, 242, 196, 255, 255, _], [99, 121, 210, 250, 201, 198, 255, 202, _, _, _], [23, 91, 163, 242, 170, 187, 247, 210, 255, 255, _]],
        [[1, 200, 246, 255, 234, 255, _, _, _, _, _], [109, 178, 241, 255, 231, 245, 255, 255, _, _, _], [44, 130, 201, 253, 205, 192, 255, 255, _, _, _]],
        [[1, 132, 239, 251, 219, 209, 255, 165, _, _, _], [94, 136, 225, 251, 218, 190, 255, 255, _, _, _], [22, 100, 174, 245, 186, 161, 255, 199, _, _, _]],
        [[1, 182, 249, 255, 232, 235, _, _, _, _, _], [124, 143, 241, 255, 227, 234, _, _, _, _, _], [35, 77, 181, 251, 193, 211, 255, 205, _, _, _]],
        [[1, 157, 247, 255, 236, 231, 255, 255, _, _, _], [121, 141, 235, 255, 225, 227, 255, 255, _, _, _], [45, 99, 188, 251, 195, 217, 255, 224, _, _, _]],
        [[1, 1, 251, 255, 213, 255, _, _, _, _, _], [203, 1, 248, 255, 255, _, _, _, _, _, _], [137, 1, 177, 255, 224, 255, _, _, _, _, _]],
    ],
    [   # block type 2: chroma
        [[253, 9, 248, 251, 207, 208, 255, 192, _, _, _], [175, 13, 224, 243, 193, 185, 249, 198, 255, 255, _], [73, 17, 171, 221, 161, 179, 236, 167, 255, 234, _]],
        [[1, 95, 247, 253, 212, 183, 255, 255, _, _, _], [239, 90, 244, 250, 211, 209, 255, 255, _, _, _], [155, 77, 195, 248, 188, 195, 255, 255, _, _, _]],
        [[1, 24, 239, 251, 218, 219, 255, 205, _, _, _], [201, 51, 219, 255, 196, 186, _, _, _, _, _], [69, 46, 190, 239, 201, 218, 255, 228, _, _, _]],
        [[1, 191, 251, 255, 255, _, _, _, _, _, _], [223, 165, 249, 255, 213, 255, _, _, _, _, _], [141, 124, 248, 255, 255, _, _, _, _, _, _]],
        [[1, 16, 248, 255, 255, _, _, _, _, _, _], [190, 36, 230, 255, 236, 255, _, _, _, _, _], [149, 1, 255, _, _, _, _, _, _, _, _]],
        [[1, 226, 255, _, _, _, _, _, _, _, _], [247, 192, 255, _, _, _, _, _, _, _, _], [240, _, 255, _, _, _, _, _, _, _, _]],
        [[1, 134, 252, 255, 255, _, _, _, _, _, _], [213, 62, 250, 255, 255, _, _, _, _, _, _], [55, 93, 255, _, _, _, _, _, _, _, _]],
        [[_] * 11, [_] * 11, [_] * 11],
    ],
    [   # block type 3: Y with DC
        [[202, 24, 213, 235, 186, 191, 220, 160, 240, 175, 255], [126, 38, 182, 232, 169, 184, 228, 174, 255, 187, _], [61, 46, 138, 219, 151, 178, 240, 170, 255, 216, _]],
        [[1, 112, 230, 250, 199, 191, 247, 159, 255, 255, _], [166, 109, 228, 252, 211, 215, 255, 174, _, _, _], [39, 77, 162, 232, 172, 180, 245, 178, 255, 255, _]],
        [[1, 52, 220, 246, 198, 199, 249, 220, 255, 255, _], [124, 74, 191, 243, 183, 193, 250, 221, 255, 255, _], [24, 71, 130, 219, 154, 170, 243, 182, 255, 255, _]],
        [[1, 182, 225, 249, 219, 240, 255, 224, _, _, _], [149, 150, 226, 252, 216, 205, 255, 171, _, _, _], [28, 108, 170, 242, 183, 194, 254, 223, 255, 255, _]],
        [[1, 81, 230, 252, 204, 203, 255, 192, _, _, _], [123, 102, 209, 247, 188, 196, 255, 233, _, _, _], [20, 95, 153, 243, 164, 173, 255, 203, _, _, _]],
        [[1, 222, 248, 255, 216, 213, _, _, _, _, _], [168, 175, 246, 252, 235, 205, 255, 255, _, _, _], [47, 116, 215, 255, 211, 212, 255, 255, _, _, _]],
        [[1, 121, 236, 253, 212, 214, 255, 255, _, _, _], [141, 84, 213, 252, 201, 202, 255, 219, _, _, _], [42, 80, 160, 240, 162, 185, 255, 205, _, _, _]],
        [[1, 1, 255, _, _, _, _, _, _, _, _], [244, 1, 255, _, _, _, _, _, _, _, _], [238, 1, 255, _, _, _, _, _, _, _, _]],
    ],
]

_ = 255
COEF_UPDATE_PROBS = [
    [
        [[_] * 11, [_] * 11, [_] * 11],
        [[176, 246, _, _, _, _, _, _, _, _, _], [223, 241, 252, _, _, _, _, _, _, _, _], [249, 253, 253, _, _, _, _, _, _, _, _]],
        [[_, 244, 252, _, _, _, _, _, _, _, _], [234, 254, 254, _, _, _, _, _, _, _, _], [253, _, _, _, _, _, _, _, _, _, _]],
        [[_, 246, 254, _, _, _, _, _, _, _, _], [239, 253, 254, _, _, _, _, _, _, _, _], [254, _, 254, _, _, _, _, _, _, _, _]],
        [[_, 248, 254, _, _, _, _, _, _, _, _], [251, _, 254, _, _, _, _, _, _, _, _], [_] * 11],
        [[_, 253, 254, _, _, _, _, _, _, _, _], [251, 254, 254, _, _, _, _, _, _, _, _], [254, _, 254, _, _, _, _, _, _, _, _]],
        [[_, 254, 253, _, 254, _, _, _, _, _, _], [250, _, 254, _, 254, _, _, _, _, _, _], [254, _, _, _, _, _, _, _, _, _, _]],
        [[_] * 11, [_] * 11, [_] * 11],
    ],
    [
        [[217, _, _, _, _, _, _, _, _, _, _], [225, 252, 241, 253, _, _, 254, _, _, _, _], [234, 250, 241, 250, 253, _, 253, 254, _, _, _]],
        [[_, 254, _, _, _, _, _, _, _, _, _], [223, 254, 254, _, _, _, _, _, _, _, _], [238, 253, 254, 254, _, _, _, _, _, _, _]],
        [[_, 248, 254, _, _, _, _, _, _, _, _], [249, 254, _, _, _, _, _, _, _, _, _], [_] * 11],
        [[_, 253, _, _, _, _, _, _, _, _, _], [247, 254, _, _, _, _, _, _, _, _, _], [_] * 11],
        [[_, 253, 254, _, _, _, _, _, _, _, _], [252, _, _, _, _, _, _, _, _, _, _], [_] * 11],
        [[_, 254, 254, _, _, _, _, _, _, _, _], [253, _, _, _, _, _, _, _, _, _, _], [_] * 11],
        [[_, 254, 253, _, _, _, _, _, _, _, _], [250, _, _, _, _, _, _, _, _, _, _], [254, _, _, _, _, _, _, _, _, _, _]],
        [[_] * 11, [_] * 11, [_] * 11],
    ],
    [
        [[186, 251, 250, _, _, _, _, _, _, _, _], [234, 251, 244, 254, _, _, _, _, _, _, _], [251, 251, 243, 253, 254, _, 254, _, _, _, _]],
        [[_, 253, 254, _, _, _, _, _, _, _, _], [236, 253, 254, _, _, _, _, _, _, _, _], [251, 253, 253, 254, 254, _, _, _, _, _, _]],
        [[_, 254, 254, _, _, _, _, _, _, _, _], [254, 254, 254, _, _, _, _, _, _, _, _], [_] * 11],
        [[_, 254, _, _, _, _, _, _, _, _, _], [254, 254, _, _, _, _, _, _, _, _, _], [254, _, _, _, _, _, _, _, _, _, _]],
        [[_] * 11, [254, _, _, _, _, _, _, _, _, _, _], [_] * 11],
        [[_] * 11, [_] * 11, [_] * 11],
        [[_] * 11, [_] * 11, [_] * 11],
        [[_] * 11, [_] * 11, [_] * 11],
    ],
    [
        [[248, _, _, _, _, _, _, _, _, _, _], [250, 254, 252, 254, _, _, _, _, _, _, _], [248, 254, 249, 253, _, _, _, _, _, _, _]],
        [[_, 253, 253, _, _, _, _, _, _, _, _], [246, 253, 253, _, _, _, _, _, _, _, _], [252, 254, 251, 254, 254, _, _, _, _, _, _]],
        [[_, 254, 252, _, _, _, _, _, _, _, _], [248, 254, 253, _, _, _, _, _, _, _, _], [253, _, 254, 254, _, _, _, _, _, _, _]],
        [[_, 251, 254, _, _, _, _, _, _, _, _], [245, 251, 254, _, _, _, _, _, _, _, _], [253, 253, 254, _, _, _, _, _, _, _, _]],
        [[_, 251, 253, _, _, _, _, _, _, _, _], [252, 253, 254, _, _, _, _, _, _, _, _], [_, 254, _, _, _, _, _, _, _, _, _]],
        [[_, 252, _, _, _, _, _, _, _, _, _], [249, _, 254, _, _, _, _, _, _, _, _], [_, _, 254, _, _, _, _, _, _, _, _]],
        [[_, _, 253, _, _, _, _, _, _, _, _], [250, _, _, _, _, _, _, _, _, _, _], [_] * 11],
        [[_] * 11, [254, _, _, _, _, _, _, _, _, _, _], [_] * 11],
    ],
]
del _

# intra modes.  16x16 luma and chroma: DC_PRED, V_PRED, H_PRED, TM_PRED, B_PRED
DC_PRED, V_PRED, H_PRED, TM_PRED, B_PRED = range(5)
# sub-block modes in the RFC's order
B_DC_PRED, B_TM_PRED, B_VE_PRED, B_HE_PRED, B_LD_PRED, B_RD_PRED, B_VR_PRED, B_VL_PRED, B_HD_PRED, B_HU_PRED = range(10)
# trees: a positive entry is the index of the next pair, a value <= 0 is minus a leaf (RFC 8.1)
KF_YMODE_TREE = [-B_PRED, 2, 4, 6, -DC_PRED, -V_PRED, -H_PRED, -TM_PRED]
KF_YMODE_PROB = [145, 156, 163, 128]
UV_MODE_TREE = [-DC_PRED, 2, -V_PRED, 4, -H_PRED, -TM_PRED]
KF_UV_MODE_PROB = [142, 114, 183]
BMODE_TREE = [-B_DC_PRED, 2, -B_TM_PRED, 4, -B_VE_PRED, 6, 8, 12, -B_HE_PRED, 10, -B_RD_PRED, -B_VR_PRED, -B_LD_PRED, 14, -B_VL_PRED, 16,
              -B_HD_PRED, -B_HU_PRED]
SEGMENT_TREE = [2, 4, -0, -1, -2, -3]
# KF_BMODE_PROBS[above][left][9]
KF_BMODE_PROBS = [
    [[231, 120, 48, 89, 115, 113, 120, 152, 112], [152, 179, 64, 126, 170, 118, 46, 70, 95], [175, 69, 143, 80, 85, 82, 72, 155, 103],
     [56, 58, 10, 171, 218, 189, 17, 13, 152], [144, 71, 10, 38, 171, 213, 144, 34, 26], [114, 26, 17, 163, 44, 195, 21, 10, 173],
     [121, 24, 80, 195, 26, 62, 44, 64, 85], [170, 46, 55, 19, 136, 160, 33, 206, 71], [63, 20, 8, 114, 114, 208, 12, 9, 226],
     [81, 40, 11, 96, 182, 84, 29, 16, 36]],
    [[134, 183, 89, 137, 98, 101, 106, 165, 148], [72, 187, 100, 130, 157, 111, 32, 75, 80], [66, 102, 167, 99, 74, 62, 40, 234, 128],
     [41, 53, 9, 178, 241, 141, 26, 8, 107], [104, 79, 12, 27, 217, 255, 87, 17, 7], [74, 43, 26, 146, 73, 166, 49, 23, 157],
     [65, 38, 105, 160, 51, 52, 31, 115, 128], [87, 68, 71, 44, 114, 51, 15, 186, 23], [47, 41, 14, 110, 182, 183, 21, 17, 194],
     [66, 45, 25, 102, 197, 189, 23, 18, 22]],
    [[88, 88, 147, 150, 42, 46, 45, 196, 205], [43, 97, 183, 117, 85, 38, 35, 179, 61], [39, 53, 200, 87, 26, 21, 43, 232, 171],
     [56, 34, 51, 104, 114, 102, 29, 93, 77], [107, 54, 32, 26, 51, 1, 81, 43, 31], [39, 28, 85, 171, 58, 165, 90, 98, 64],
     [34, 22, 116, 206, 23, 34, 43, 166, 73], [68, 25, 106, 22, 64, 171, 36, 225, 114], [34, 19, 21, 102, 132, 188, 16, 76, 124],
     [62, 18, 78, 95, 85, 57, 50, 48, 51]],
    [[193, 101, 35, 159, 215, 111, 89, 46, 111], [60, 148, 31, 172, 219, 228, 21, 18, 111], [112, 113, 77, 85, 179, 255, 38, 120, 114],
     [40, 42, 1, 196, 245, 209, 10, 25, 109], [100, 80, 8, 43, 154, 1, 51, 26, 71], [88, 43, 29, 140, 166, 213, 37, 43, 154],
     [61, 63, 30, 155, 67, 45, 68, 1, 209], [142, 78, 78, 16, 255, 128, 34, 197, 171], [41, 40, 5, 102, 211, 183, 4, 1, 221],
     [51, 50, 17, 168, 209, 192, 23, 25, 82]],
    [[125, 98, 42, 88, 104, 85, 117, 175, 82], [95, 84, 53, 89, 128, 100, 113, 101, 45], [75, 79, 123, 47, 51, 128, 81, 171, 1],
     [57, 17, 5, 71, 102, 57, 53, 41, 49], [115, 21, 2, 10, 102, 255, 166, 23, 6], [38, 33, 13, 121, 57, 73, 26, 1, 85],
     [41, 10, 67, 138, 77, 110, 90, 47, 114], [101, 29, 16, 10, 85, 128, 101, 196, 26], [57, 18, 10, 102, 102, 213, 34, 20, 43],
     [117, 20, 15, 36, 163, 128, 68, 1, 26]],
    [[138, 31, 36, 171, 27, 166, 38, 44, 229], [67, 87, 58, 169, 82, 115, 26, 59, 179], [63, 59, 90, 180, 59, 166, 93, 73, 154],
     [40, 40, 21, 116, 143, 209, 34, 39, 175], [57, 46, 22, 24, 128, 1, 54, 17, 37], [47, 15, 16, 183, 34, 223, 49, 45, 183],
     [46, 17, 33, 183, 6, 98, 15, 32, 183], [65, 32, 73, 115, 28, 128, 23, 128, 205], [40, 3, 9, 115, 51, 192, 18, 6, 223],
     [87, 37, 9, 115, 59, 77, 64, 21, 47]],
    [[104, 55, 44, 218, 9, 54, 53, 130, 226], [64, 90, 70, 205, 40, 41, 23, 26, 57], [54, 57, 112, 184, 5, 41, 38, 166, 213],
     [30, 34, 26, 133, 152, 116, 10, 32, 134], [75, 32, 12, 51, 192, 255, 160, 43, 51], [39, 19, 53, 221, 26, 114, 32, 73, 255],
     [31, 9, 65, 234, 2, 15, 1, 118, 73], [88, 31, 35, 67, 102, 85, 55, 186, 85], [56, 21, 23, 111, 59, 205, 45, 37, 192],
     [55, 38, 70, 124, 73, 102, 1, 34, 98]],
    [[102, 61, 71, 37, 34, 53, 31, 243, 192], [69, 60, 71, 38, 73, 119, 28, 222, 37], [68, 45, 128, 34, 1, 47, 11, 245, 171],
     [62, 17, 19, 70, 146, 85, 55, 62, 70], [75, 15, 9, 9, 64, 255, 184, 119, 16], [37, 43, 37, 154, 100, 163, 85, 160, 1],
     [63, 9, 92, 136, 28, 64, 32, 201, 85], [86, 6, 28, 5, 64, 255, 25, 248, 1], [56, 8, 17, 132, 137, 255, 55, 116, 128],
     [58, 15, 20, 82, 135, 57, 26, 121, 40]],
    [[164, 50, 31, 137, 154, 133, 25, 35, 218], [51, 103, 44, 131, 131, 123, 31, 6, 158], [86, 40, 64, 135, 148, 224, 45, 183, 128],
     [22, 26, 17, 131, 240, 154, 14, 1, 209], [83, 12, 13, 54, 192, 255, 68, 47, 28], [45, 16, 21, 91, 64, 222, 7, 1, 197],
     [56, 21, 39, 155, 60, 138, 23, 102, 213], [85, 26, 85, 85, 128, 128, 32, 146, 171], [18, 11, 7, 63, 144, 171, 4, 4, 246],
     [35, 27, 10, 146, 174, 171, 12, 26, 128]],
    [[190, 80, 35, 99, 180, 80, 126, 54, 45], [85, 126, 47, 87, 176, 51, 41, 20, 32], [101, 75, 128, 139, 118, 146, 116, 128, 85],
     [56, 41, 15, 176, 236, 85, 37, 9, 62], [146, 36, 19, 30, 171, 255, 97, 27, 20], [71, 30, 17, 119, 118, 255, 17, 18, 138],
     [101, 38, 60, 138, 55, 70, 43, 26, 142], [138, 45, 61, 62, 219, 1, 81, 188, 64], [32, 41, 20, 117, 151, 142, 20, 21, 163],
     [112, 19, 12, 61, 195, 128, 48, 4, 24]],
]

# tokens (RFC 13.2)
DCT_0, DCT_1, DCT_2, DCT_3, DCT_4, DCT_CAT1, DCT_CAT2, DCT_CAT3, DCT_CAT4, DCT_CAT5, DCT_CAT6, DCT_EOB = range(12)
COEF_TREE = [-DCT_EOB, 2, -DCT_0, 4, -DCT_1, 6, 8, 12, -DCT_2, 10, -DCT_3, -DCT_4, 14, 16, -DCT_CAT1, -DCT_CAT2, 18, 20, -DCT_CAT3, -DCT_CAT4,
             -DCT_CAT5, -DCT_CAT6]
CAT_BASE = [5, 7, 11, 19, 35, 67]
CAT_PROBS = [[159], [165, 145], [173, 148, 140], [176, 155, 140, 135], [180, 157, 141, 134, 130], [254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129]]
COEF_BANDS = [0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7]
ZIGZAG = [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15]
# a non-B_PRED macroblock stands for this sub-block mode in its neighbours' contexts (RFC 11.3)
IMPLIED_BMODE = {DC_PRED: B_DC_PRED, V_PRED: B_VE_PRED, H_PRED: B_HE_PRED, TM_PRED: B_TM_PRED}


class BoolDecoder:
    """RFC 7.3, with zeros past the end of the data; `past` counts those bytes."""

    def __init__(self, data):
        self.data, self.pos, self.past = data, 0, 0
        self.value = self._byte() << 8 | self._byte()
        self.range, self.bit_count = 255, 0

    def _byte(self):
        if self.pos < len(self.data):
            b = self.data[self.pos]
        else:
            b = 0
            self.past += 1
        self.pos += 1
        return b

    def read(self, prob):
        split = 1 + (((self.range - 1) * prob) >> 8)
        big = split << 8
        if self.value >= big:
            bit = 1
            self.range -= split
            self.value -= big
        else:
            bit = 0
            self.range = split
        while self.range < 128:
            self.value <<= 1
            self.range <<= 1
            self.bit_count += 1
            if self.bit_count == 8:
                self.bit_count = 0
                self.value |= self._byte()
        return bit

    def literal(self, n):
        v = 0
        for _i in range(n):
            v = v << 1 | self.read(128)
        return v

    def flagged(self, n):
        """an optional signed value: flag, n-bit magnitude, sign"""
        if not self.read(128):
            return 0
        v = self.literal(n)
        return -v if self.read(128) else v

    def tree(self, tree, probs, start=0):
        i = start
        while True:
            i = tree[i + self.read(probs[i >> 1])]
            if i <= 0:
                return -i


def clamp255(v):
    return 0 if v < 0 else 255 if v > 255 else v


def s16(v):
    return ((v + 32768) & 65535) - 32768


def iwht(c):
    """RFC 14.3: the 16 DC values of the luma blocks from the Y2 block (exact for a lone DC too)"""
    t = [0] * 16
    for i in range(4):
        a1, b1 = c[i] + c[12 + i], c[4 + i] + c[8 + i]
        c1, d1 = c[4 + i] - c[8 + i], c[i] - c[12 + i]
        t[i], t[4 + i], t[8 + i], t[12 + i] = a1 + b1, c1 + d1, a1 - b1, d1 - c1
    out = [0] * 16
    for i in range(4):
        a1, b1 = t[4 * i] + t[4 * i + 3], t[4 * i + 1] + t[4 * i + 2]
        c1, d1 = t[4 * i + 1] - t[4 * i + 2], t[4 * i] - t[4 * i + 3]
        out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3] = (a1 + b1 + 3) >> 3, (c1 + d1 + 3) >> 3, (a1 - b1 + 3) >> 3, (d1 - c1 + 3) >> 3
    return [s16(v) for v in out]


def idct(c):
    """RFC 14.3: residual[16] (row major) of one 4x4 block"""
    t = [0] * 16
    for i in range(4):
        a1, b1 = c[i] + c[8 + i], c[i] - c[8 + i]
        c1 = ((c[4 + i] * 35468) >> 16) - (c[12 + i] + ((c[12 + i] * 20091) >> 16))
        d1 = (c[4 + i] + ((c[4 + i] * 20091) >> 16)) + ((c[12 + i] * 35468) >> 16)
        t[i], t[4 + i], t[8 + i], t[12 + i] = s16(a1 + d1), s16(b1 + c1), s16(b1 - c1), s16(a1 - d1)      # (the RFC keeps them in 16-bit words)
    out = [0] * 16
    for i in range(4):
        r = t[4 * i:4 * i + 4]
        a1, b1 = r[0] + r[2], r[0] - r[2]
        c1 = ((r[1] * 35468) >> 16) - (r[3] + ((r[3] * 20091) >> 16))
        d1 = (r[1] + ((r[1] * 20091) >> 16)) + ((r[3] * 35468) >> 16)
        out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3] = (a1 + d1 + 4) >> 3, (b1 + c1 + 4) >> 3, (b1 - c1 + 4) >> 3, (a1 - d1 + 4) >> 3
    return out


def predict_block(mode, A, L, P):
    """RFC 12.3: a 4x4 sub-block from the 8 samples above / above right, the 4 to the left and the corner; B[row][col]"""
    def a3(x, y, z):
        return (x + 2 * y + z + 2) >> 2

    def a2(x, y):
        return (x + y + 1) >> 1
    E = [L[3], L[2], L[1], L[0], P] + list(A)
    B = [[0] * 4 for _i in range(4)]
    if mode == B_DC_PRED:
        v = (sum(A[:4]) + sum(L) + 4) >> 3
        B = [[v] * 4 for _i in range(4)]
    elif mode == B_TM_PRED:
        B = [[clamp255(L[r] + A[c] - P) for c in range(4)] for r in range(4)]
    elif mode == B_VE_PRED:
        row = [a3(P, A[0], A[1]), a3(A[0], A[1], A[2]), a3(A[1], A[2], A[3]), a3(A[2], A[3], A[4])]
        B = [list(row) for _i in range(4)]
    elif mode == B_HE_PRED:
        col = [a3(P, L[0], L[1]), a3(L[0], L[1], L[2]), a3(L[1], L[2], L[3]), a3(L[2], L[3], L[3])]
        B = [[col[r]] * 4 for r in range(4)]
    elif mode == B_LD_PRED:
        for r in range(4):
            for c in range(4):
                i = r + c
                B[r][c] = a3(A[i], A[i + 1], A[min(i + 2, 7)])
    elif mode == B_RD_PRED:
        for r in range(4):
            for c in range(4):
                i = 4 - r + c
                B[r][c] = a3(E[i - 1], E[i], E[i + 1])
    elif mode == B_VR_PRED:
        B[3][0] = a3(E[1], E[2], E[3])
        B[2][0] = a3(E[2], E[3], E[4])
        B[3][1] = B[1][0] = a3(E[3], E[4], E[5])
        B[2][1] = B[0][0] = a2(E[4], E[5])
        B[3][2] = B[1][1] = a3(E[4], E[5], E[6])
        B[2][2] = B[0][1] = a2(E[5], E[6])
        B[3][3] = B[1][2] = a3(E[5], E[6], E[7])
        B[2][3] = B[0][2] = a2(E[6], E[7])
        B[1][3] = a3(E[6], E[7], E[8])
        B[0][3] = a2(E[7], E[8])
    elif mode == B_VL_PRED:
        B[0][0] = a2(A[0], A[1])
        B[1][0] = a3(A[0], A[1], A[2])
        B[2][0] = B[0][1] = a2(A[1], A[2])
        B[1][1] = B[3][0] = a3(A[1], A[2], A[3])
        B[2][1] = B[0][2] = a2(A[2], A[3])
        B[3][1] = B[1][2] = a3(A[2], A[3], A[4])
        B[2][2] = B[0][3] = a2(A[3], A[4])
        B[3][2] = B[1][3] = a3(A[3], A[4], A[5])
        B[2][3] = a3(A[4], A[5], A[6])
        B[3][3] = a3(A[5], A[6], A[7])
    elif mode == B_HD_PRED:
        B[3][0] = a2(E[0], E[1])
        B[3][1] = a3(E[0], E[1], E[2])
        B[2][0] = B[3][2] = a2(E[1], E[2])
        B[2][1] = B[3][3] = a3(E[1], E[2], E[3])
        B[2][2] = B[1][0] = a2(E[2], E[3])
        B[2][3] = B[1][1] = a3(E[2], E[3], E[4])
        B[1][2] = B[0][0] = a2(E[3], E[4])
        B[1][3] = B[0][1] = a3(E[3], E[4], E[5])
        B[0][2] = a3(E[4], E[5], E[6])
        B[0][3] = a3(E[5], E[6], E[7])
    elif mode == B_HU_PRED:
        B[0][0] = a2(L[0], L[1])
        B[0][1] = a3(L[0], L[1], L[2])
        B[0][2] = B[1][0] = a2(L[1], L[2])
        B[0][3] = B[1][1] = a3(L[1], L[2], L[3])
        B[1][2] = B[2][0] = a2(L[2], L[3])
        B[1][3] = B[2][1] = a3(L[2], L[3], L[3])
        B[2][2] = B[2][3] = B[3][0] = B[3][1] = B[3][2] = B[3][3] = L[3]
    else:
        raise ValueError(mode)
    return B


def predict_mb(mode, n, above, left, corner, has_above, has_left):
    """RFC 12.2: an n x n prediction (16 luma, 8 chroma) from the row above, the column to the left and the corner (127 / 129 outside the frame)"""
    if mode == DC_PRED:
        shift = 3 if n == 8 else 4
        if has_above and has_left:
            v = (sum(above) + sum(left) + (1 << shift)) >> (shift + 1)
        elif has_above:
            v = (sum(above) + (1 << (shift - 1))) >> shift
        elif has_left:
            v = (sum(left) + (1 << (shift - 1))) >> shift
        else:
            v = 128
        return [[v] * n for _i in range(n)]
    if mode == V_PRED:
        return [list(above) for _i in range(n)]
    if mode == H_PRED:
        return [[left[r]] * n for r in range(n)]
    if mode == TM_PRED:
        return [[clamp255(left[r] + above[c] - corner) for c in range(n)] for r in range(n)]
    raise ValueError(mode)


# ---- loop filter (RFC 15) ----
def _c(v):
    return -128 if v < -128 else 127 if v > 127 else v


def _common_adjust(use_outer, px, i, st):
    p1, p0, q0, q1 = px[i - 2 * st] - 128, px[i - st] - 128, px[i] - 128, px[i + st] - 128
    a = _c((_c(p1 - q1) if use_outer else 0) + 3 * (q0 - p0))
    b = _c(a + 3) >> 3
    a = _c(a + 4) >> 3
    px[i] = _c(q0 - a) + 128
    px[i - st] = _c(p0 + b) + 128
    return a


def _simple_threshold(px, i, st, limit):
    return abs(px[i - st] - px[i]) * 2 + (abs(px[i - 2 * st] - px[i + st]) >> 1) <= limit


def filter_simple(px, i, st, limit):
    if _simple_threshold(px, i, st, limit):
        _common_adjust(True, px, i, st)


def _normal_yes(px, i, st, interior, limit):
    p3, p2, p1, p0 = px[i - 4 * st], px[i - 3 * st], px[i - 2 * st], px[i - st]
    q0, q1, q2, q3 = px[i], px[i + st], px[i + 2 * st], px[i + 3 * st]
    return (abs(p0 - q0) * 2 + (abs(p1 - q1) >> 1) <= limit and abs(p3 - p2) <= interior and abs(p2 - p1) <= interior and abs(p1 - p0) <= interior
            and abs(q3 - q2) <= interior and abs(q2 - q1) <= interior and abs(q1 - q0) <= interior)


def _hev(px, i, st, thresh):
    return abs(px[i - 2 * st] - px[i - st]) > thresh or abs(px[i + st] - px[i]) > thresh


def filter_subblock(px, i, st, interior, limit, thresh):
    if not _normal_yes(px, i, st, interior, limit):
        return
    hv = _hev(px, i, st, thresh)
    p1, q1 = px[i - 2 * st] - 128, px[i + st] - 128
    a = (_common_adjust(hv, px, i, st) + 1) >> 1
    if not hv:
        px[i + st] = _c(q1 - a) + 128
        px[i - 2 * st] = _c(p1 + a) + 128


def filter_mbedge(px, i, st, interior, limit, thresh):
    if not _normal_yes(px, i, st, interior, limit):
        return
    if _hev(px, i, st, thresh):
        _common_adjust(True, px, i, st)
        return
    p2, p1, p0 = px[i - 3 * st] - 128, px[i - 2 * st] - 128, px[i - st] - 128
    q0, q1, q2 = px[i] - 128, px[i + st] - 128, px[i + 2 * st] - 128
    w = _c(_c(p1 - q1) + 3 * (q0 - p0))
    a = _c((27 * w + 63) >> 7)
    px[i], px[i - st] = _c(q0 - a) + 128, _c(p0 + a) + 128
    a = _c((18 * w + 63) >> 7)
    px[i + st], px[i - 2 * st] = _c(q1 - a) + 128, _c(p1 + a) + 128
    a = _c((9 * w + 63) >> 7)
    px[i + 2 * st], px[i - 3 * st] = _c(q2 - a) + 128, _c(p2 + a) + 128


def filter_limits(level, sharpness):
    """(interior limit, sub-block edge limit, macroblock edge limit, key-frame hev threshold) of a filter level (RFC 15.2, 15.3)"""
    interior = level
    if sharpness:
        interior >>= 2 if sharpness > 4 else 1
        interior = min(interior, 9 - sharpness)
    interior = max(interior, 1)
    return interior, level * 2 + interior, (level + 2) * 2 + interior, 2 if level >= 40 else 1 if level >= 15 else 0


class Header:
    pass


class RefDecoder:
    def __init__(self):
        self.errors = 0
        self.key_frames = self.hidden = self.empty = 0
        self.width = self.height = 0
        self.info = dict(ymodes=set(), uvmodes=set(), bmodes=set(), segments=set(), partitions=set(), filter_types=set(), levels=set(), skipped_mbs=0,
                         coded_mbs=0, bpred_mbs=0, cats=set(), mb_edge_mbs=0, inner_edge_mbs=0, damaged=0, versions=set(), sharpness=set(),
                         color_space=set(), clamping=set(), scale=set(), no_coeff_skip=set(), seg_abs=set(), lf_delta=set(), prob_updates=0,
                         q_deltas=set(), refresh=set(), max_past=0)

    # -- one frame -> (planes, w, h, shown) or None for an empty frame
    def decode_frame(self, f):
        info = self.info
        if len(f) == 0:
            self.empty += 1
            return None
        damaged = False
        if len(f) < 3:
            f = bytes(f) + bytes(3 - len(f))
            damaged = True
        tag = f[0] | f[1] << 8 | f[2] << 16
        key, version, show, part1 = not (tag & 1), tag >> 1 & 7, tag >> 4 & 1, tag >> 5
        if not key:
            raise Refused("VP8 inter frames are not built" if self.key_frames else "VP8: the first frame is not a key frame")
        if version > 3:
            raise Refused("VP8: version %d is not defined (RFC 6386 9.1)" % version)
        hdr = bytes(f[3:10]) + bytes(max(0, 10 - len(f)))
        if len(f) < 10:
            damaged = True
        if hdr[0:3] != b"\x9d\x01\x2a":
            raise Refused("VP8: bad start code")
        w, hs = (hdr[3] | hdr[4] << 8) & 0x3FFF, hdr[4] >> 6
        h, vs = (hdr[5] | hdr[6] << 8) & 0x3FFF, hdr[6] >> 6
        if w == 0 or h == 0 or w > MAX_DIM or h > MAX_DIM:
            raise Refused("VP8: picture size %dx%d is not supported" % (w, h))
        info["versions"].add(version)
        info["scale"].add((hs, vs))
        body = f[10:]
        if part1 > len(body):
            damaged = True
        d = BoolDecoder(body[:part1])
        H = Header()
        H.color_space, H.clamping = d.literal(1), d.literal(1)
        info["color_space"].add(H.color_space)
        info["clamping"].add(H.clamping)
        # segmentation (9.3): a key frame starts from nothing
        seg_q, seg_lf, seg_abs, seg_probs = [0] * 4, [0] * 4, 0, [255] * 3
        seg_on = d.literal(1)
        update_map = 0
        if seg_on:
            update_map = d.literal(1)
            if d.literal(1):
                seg_abs = d.literal(1)
                seg_q = [d.flagged(7) for _i in range(4)]
                seg_lf = [d.flagged(6) for _i in range(4)]
                info["seg_abs"].add(seg_abs)
            if update_map:
                seg_probs = [d.literal(8) if d.literal(1) else 255 for _i in range(3)]
        # loop filter (9.6)
        filter_type, level, sharpness = d.literal(1), d.literal(6), d.literal(3)
        ref_delta, mode_delta = [0] * 4, [0] * 4
        delta_on = d.literal(1)
        if delta_on:
            if d.literal(1):
                ref_delta = [d.flagged(6) for _i in range(4)]
                mode_delta = [d.flagged(6) for _i in range(4)]
                info["lf_delta"].add((ref_delta[0], mode_delta[0]))
        info["filter_types"].add(filter_type)
        info["sharpness"].add(sharpness)
        n_parts = 1 << d.literal(2)
        info["partitions"].add(n_parts)
        # quantiser (9.6)
        yac = d.literal(7)
        ydc, y2dc, y2ac, uvdc, uvac = [d.flagged(4) for _i in range(5)]
        info["q_deltas"].add((ydc, y2dc, y2ac, uvdc, uvac))
        info["refresh"].add(d.literal(1))          # refresh_entropy_probs: the next key frame starts from the defaults either way
        probs = [[[list(c) for c in b] for b in t] for t in DEFAULT_COEF_PROBS]
        for i in range(4):
            for j in range(8):
                for k in range(3):
                    for l in range(11):
                        if d.read(COEF_UPDATE_PROBS[i][j][k][l]):
                            probs[i][j][k][l] = d.literal(8)
                            info["prob_updates"] += 1
        no_coeff_skip = d.literal(1)
        prob_skip = d.literal(8) if no_coeff_skip else 0
        info["no_coeff_skip"].add(no_coeff_skip)

        def q(i):
            return 0 if i < 0 else 127 if i > 127 else i
        dq = []
        for s in range(4):
            base = yac
            if seg_on:
                base = seg_q[s] if seg_abs else yac + seg_q[s]
            base = q(base)
            dq.append((DC_Q[q(base + ydc)], AC_Q[base], DC_Q[q(base + y2dc)] * 2, max(AC_Q[q(base + y2ac)] * 155 // 100, 8), min(DC_Q[q(base + uvdc)], 132),
                       AC_Q[q(base + uvac)]))
        # token partitions (9.5)
        rest = body[part1:]
        sizes_len = 3 * (n_parts - 1)
        if len(rest) < sizes_len:
            damaged = True
        sizes = bytes(rest[:sizes_len]) + bytes(max(0, sizes_len - len(rest)))
        rest = rest[sizes_len:]
        parts, o = [], 0
        for p in range(n_parts):
            n = sizes[3 * p] | sizes[3 * p + 1] << 8 | sizes[3 * p + 2] << 16 if p < n_parts - 1 else max(0, len(rest) - o)
            if o + n > len(rest):
                damaged = True
            parts.append(BoolDecoder(rest[o:o + n]))
            o += n

        mbw, mbh = (w + 15) >> 4, (h + 15) >> 4
        Y = np.zeros((mbh * 16, mbw * 16), np.int32)
        U = np.zeros((mbh * 8, mbw * 8), np.int32)
        V = np.zeros((mbh * 8, mbw * 8), np.int32)
        above_b = [[B_DC_PRED] * 4 for _i in range(mbw)]     # sub-block modes of the bottom row of the macroblocks above
        # non-zero contexts: 4 Y, 2 U, 2 V, 1 Y2 per macroblock column / for the macroblock to the left
        above_nz = [[0] * 9 for _i in range(mbw)]
        mbs = []
        for my in range(mbh):
            left_b = [B_DC_PRED] * 4
            left_nz = [0] * 9
            tok = parts[my % n_parts]
            for mx in range(mbw):
                m = Header()
                m.segment = d.tree(SEGMENT_TREE, seg_probs) if update_map else 0
                m.skip = d.read(prob_skip) if no_coeff_skip else 0
                m.ymode = d.tree(KF_YMODE_TREE, KF_YMODE_PROB)
                if m.ymode == B_PRED:
                    m.bmodes = []
                    for b in range(16):
                        A = above_b[mx][b & 3] if b < 4 else m.bmodes[b - 4]
                        L = left_b[b >> 2] if not (b & 3) else m.bmodes[b - 1]
                        m.bmodes.append(d.tree(BMODE_TREE, KF_BMODE_PROBS[A][L]))
                    info["bmodes"].update(m.bmodes)
                    info["bpred_mbs"] += 1
                else:
                    m.bmodes = [IMPLIED_BMODE[m.ymode]] * 16
                above_b[mx] = m.bmodes[12:16]
                left_b = m.bmodes[3::4]
                m.uvmode = d.tree(UV_MODE_TREE, KF_UV_MODE_PROB)
                info["ymodes"].add(m.ymode)
                info["uvmodes"].add(m.uvmode)
                if seg_on:
                    info["segments"].add(m.segment)
                # residual data (13)
                coef = [[0] * 16 for _i in range(25)]
                any_nz = False
                an, ln = above_nz[mx], left_nz
                if m.skip:
                    info["skipped_mbs"] += 1
                    keep_a, keep_l = an[8], ln[8]
                    an[:] = [0] * 9
                    ln[:] = [0] * 9
                    if m.ymode == B_PRED:
                        an[8], ln[8] = keep_a, keep_l
                else:
                    info["coded_mbs"] += 1
                    D = dq[m.segment]
                    first = 0
                    if m.ymode != B_PRED:
                        nz = self._block(tok, probs[1], an[8] + ln[8], 0, coef[24], D[2], D[3])
                        an[8] = ln[8] = nz
                        any_nz |= bool(nz)
                        first = 1
                    ptype = 0 if first else 3
                    for b in range(16):
                        nz = self._block(tok, probs[ptype], an[b & 3] + ln[b >> 2], first, coef[b], D[0], D[1])
                        an[b & 3] = ln[b >> 2] = nz
                        any_nz |= bool(nz)
                    for c in range(2):
                        for b in range(4):
                            ia, il = 4 + 2 * c + (b & 1), 4 + 2 * c + (b >> 1)
                            nz = self._block(tok, probs[2], an[ia] + ln[il], 0, coef[16 + 4 * c + b], D[4], D[5])
                            an[ia] = ln[il] = nz
                            any_nz |= bool(nz)
                m.inner = m.ymode == B_PRED or any_nz
                # filter level (9.3, 9.6, 15.1-15.3: only the intra-frame and B_PRED deltas can apply on a key frame)
                lv = level
                if seg_on:
                    lv = seg_lf[m.segment] if seg_abs else level + seg_lf[m.segment]
                lv = min(max(lv, 0), 63)
                if delta_on:
                    lv += ref_delta[0]
                    if m.ymode == B_PRED:
                        lv += mode_delta[0]
                    lv = min(max(lv, 0), 63)
                m.level = lv
                info["levels"].add(lv)
                mbs.append(m)
                self._reconstruct(m, coef, Y, U, V, mx, my, mbw)
        past = max([d.past] + [p.past for p in parts])
        info["max_past"] = max(info["max_past"], past)
        if past > 2:
            damaged = True
        if damaged:
            self.errors += 1
            info["damaged"] += 1
        # loop filter over the finished reconstruction (15)
        planes = [Y.reshape(-1).tolist(), U.reshape(-1).tolist(), V.reshape(-1).tolist()]
        strides = [mbw * 16, mbw * 8, mbw * 8]
        for my in range(mbh):
            for mx in range(mbw):
                m = mbs[my * mbw + mx]
                if not m.level:
                    continue
                interior, sub_limit, mb_limit, thresh = filter_limits(m.level, sharpness)
                if mx or my:
                    info["mb_edge_mbs"] += 1
                if m.inner:
                    info["inner_edge_mbs"] += 1
                for pl in range(1 if filter_type else 3):
                    n, st = (16 if pl == 0 else 8), strides[pl]
                    px, o = planes[pl], my * n * st + mx * n
                    if mx:
                        for r in range(n):
                            if filter_type:
                                filter_simple(px, o + r * st, 1, mb_limit)
                            else:
                                filter_mbedge(px, o + r * st, 1, interior, mb_limit, thresh)
                    if m.inner:
                        for e in range(4, n, 4):
                            for r in range(n):
                                if filter_type:
                                    filter_simple(px, o + r * st + e, 1, sub_limit)
                                else:
                                    filter_subblock(px, o + r * st + e, 1, interior, sub_limit, thresh)
                    if my:
                        for c in range(n):
                            if filter_type:
                                filter_simple(px, o + c, st, mb_limit)
                            else:
                                filter_mbedge(px, o + c, st, interior, mb_limit, thresh)
                    if m.inner:
                        for e in range(4, n, 4):
                            for c in range(n):
                                if filter_type:
                                    filter_simple(px, o + e * st + c, st, sub_limit)
                                else:
                                    filter_subblock(px, o + e * st + c, st, interior, sub_limit, thresh)
        out = [np.array(planes[0], np.uint8).reshape(mbh * 16, mbw * 16), np.array(planes[1], np.uint8).reshape(mbh * 8, mbw * 8),
               np.array(planes[2], np.uint8).reshape(mbh * 8, mbw * 8)]
        self.key_frames += 1
        if not show:
            self.hidden += 1
        self.width, self.height = w, h
        return out, w, h, bool(show)

    def _block(self, d, probs, ctx, first, out, dcq, acq):
        """the tokens of one block (13.2-13.3); out[] gets dequantised coefficients at their raster positions; -> 1 when any token but EOB was read"""
        i, start = first, 0
        while i < 16:
            t = d.tree(COEF_TREE, probs[COEF_BANDS[i]][ctx], start)
            if t == DCT_EOB:
                break
            if t == DCT_0:
                ctx, start = 0, 2          # (no EOB can follow a zero: the tree is entered past its first branch)
                i += 1
                continue
            if t <= DCT_4:
                v = t
            else:
                c = t - DCT_CAT1
                self.info["cats"].add(c + 1)
                extra = 0
                for p in CAT_PROBS[c]:
                    extra = extra << 1 | d.read(p)
                v = CAT_BASE[c] + extra
            ctx = 1 if v == 1 else 2
            if d.read(128):
                v = -v
            out[ZIGZAG[i]] = s16(v * (acq if i else dcq))
            start = 0
            i += 1
        return 1 if i > first else 0

    def _reconstruct(self, m, coef, Y, U, V, mx, my, mbw):
        x0, y0 = mx * 16, my * 16
        if m.ymode != B_PRED:
            dc = iwht(coef[24])
            for b in range(16):
                coef[b][0] = dc[b]
            above = Y[y0 - 1, x0:x0 + 16].tolist() if my else [127] * 16
            left = Y[y0:y0 + 16, x0 - 1].tolist() if mx else [129] * 16
            corner = (int(Y[y0 - 1, x0 - 1]) if mx else 129) if my else 127
            P = predict_mb(m.ymode, 16, above, left, corner, my > 0, mx > 0)
            for b in range(16):
                r = idct(coef[b])
                bx, by = (b & 3) * 4, (b >> 2) * 4
                for i in range(4):
                    for j in range(4):
                        Y[y0 + by + i, x0 + bx + j] = clamp255(P[by + i][bx + j] + r[4 * i + j])
        else:
            # the row above the macroblock, with its 4 above-right samples
            if my == 0:
                row = [127] * 20
            else:
                row = Y[y0 - 1, x0:x0 + 16].tolist()
                row += Y[y0 - 1, x0 + 16:x0 + 20].tolist() if mx < mbw - 1 else [row[15]] * 4
            for b in range(16):
                bx, by = (b & 3) * 4, (b >> 2) * 4
                if by == 0:
                    A = row[bx:bx + 8]
                else:
                    A = Y[y0 + by - 1, x0 + bx:x0 + bx + 4].tolist()
                    A += Y[y0 + by - 1, x0 + bx + 4:x0 + bx + 8].tolist() if bx < 12 else row[16:20]
                L = Y[y0 + by:y0 + by + 4, x0 + bx - 1].tolist() if (mx or bx) else [129] * 4
                if by:
                    P = int(Y[y0 + by - 1, x0 + bx - 1]) if (mx or bx) else 129
                elif my:
                    P = int(Y[y0 - 1, x0 + bx - 1]) if (mx or bx) else 129
                else:
                    P = 127
                B = predict_block(m.bmodes[b], A, L, P)
                r = idct(coef[b])
                for i in range(4):
                    for j in range(4):
                        Y[y0 + by + i, x0 + bx + j] = clamp255(B[i][j] + r[4 * i + j])
        x0, y0 = mx * 8, my * 8
        for c, pl in enumerate((U, V)):
            above = pl[y0 - 1, x0:x0 + 8].tolist() if my else [127] * 8
            left = pl[y0:y0 + 8, x0 - 1].tolist() if mx else [129] * 8
            corner = (int(pl[y0 - 1, x0 - 1]) if mx else 129) if my else 127
            P = predict_mb(m.uvmode, 8, above, left, corner, my > 0, mx > 0)
            for b in range(4):
                r = idct(coef[16 + 4 * c + b])
                bx, by = (b & 1) * 4, (b >> 1) * 4
                for i in range(4):
                    for j in range(4):
                        pl[y0 + by + i, x0 + bx + j] = clamp255(P[by + i][bx + j] + r[4 * i + j])


def webp_payload(data):
    """The `VP8 ` chunk of a RIFF / WebP file (lossy, no alpha)."""
    data = bytes(data)
    assert data[:4] == b"RIFF" and data[8:12] == b"WEBP", "not a WebP file"
    o = 12
    while o + 8 <= len(data):
        tag, n = data[o:o + 4], struct.unpack_from("<I", data, o + 4)[0]
        if tag == b"VP8 ":
            return data[o + 8:o + 8 + n]
        o += 8 + n + (n & 1)
    raise ValueError("no VP8 chunk")


def ivf(frames, width=0, height=0):
    """An IVF byte stream of the frames."""
    out = b"DKIF" + struct.pack("<HH4sHHIIII", 0, 32, b"VP80", width, height, 30, 1, len(frames), 0)
    for i, f in enumerate(frames):
        out += struct.pack("<IQ", len(f), i) + bytes(f)
    return out


def split_ivf(data):
    """The frames of an IVF byte stream; a frame cut off by the end of the stream is kept as far as it goes."""
    data = bytes(data)
    frames, o = [], 32
    while o + 12 <= len(data):
        n = struct.unpack_from("<I", data, o)[0]
        frames.append(data[o + 12:o + 12 + n])
        o += 12 + n
    return frames


def nv12(planes, width, height):
    dw, dh = (width + 1) & ~1, (height + 1) & ~1
    f = np.zeros((dh * 3 // 2, dw), np.uint8)
    f[:dh] = planes[0][:dh, :dw]
    f[dh:, 0::2] = planes[1][:dh // 2, :dw // 2]
    f[dh:, 1::2] = planes[2][:dh // 2, :dw // 2]
    return f, dw, dh


def decode_planes(frame):
    """One key frame -> (Y, U, V cropped to the display size the way libwebp hands them out, info)."""
    d = RefDecoder()
    planes, w, h, _shown = d.decode_frame(frame)
    d.info["errors"] = d.errors
    return planes[0][:h, :w], planes[1][:(h + 1) // 2, :(w + 1) // 2], planes[2][:(h + 1) // 2, :(w + 1) // 2], d.info


def decode_stream(data, out_fmt=1, info=None):
    """Every display frame of a stream -> [(frame bytes, dw, dh)].  data: an IVF byte stream, or a list of frames (one per call).  A refusal raises
    Refused after info has been filled with what was decoded before it."""
    d = RefDecoder()
    out = []
    frames = split_ivf(data) if isinstance(data, (bytes, bytearray)) and bytes(data[:4]) == b"DKIF" else ([data] if isinstance(data, (bytes, bytearray)) else list(data))
    try:
        for f in frames:
            r = d.decode_frame(f)
            if r is None or not r[3]:
                continue
            fr, dw, dh = nv12(r[0], r[1], r[2])
            out.append((frame_bytes(fr, dw, dh, out_fmt), dw, dh))
    finally:
        if info is not None:
            info.update(d.info)
            info.update(errors=d.errors, key_frames=d.key_frames, hidden=d.hidden, empty=d.empty)
    return out
