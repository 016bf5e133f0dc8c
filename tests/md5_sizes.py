"""Sizes for the MD5 tests (test_md5_host.py, test_md5_gpu.py) -- a helper, not a test.  TILE restates md5::kMd5TileBytes (jmcodec_amd/csrc/md5_packed.h)
as a literal: test_md5_host.py asserts that tools/md5_asan prints the same number, so the sizes below that sit on a tile boundary cannot silently stop
doing so when the kernel's tile changes."""
TILE = 4096
T = TILE

# stream lengths for md5_asan's raw mode: around the 56-byte point where the length field spills into a second block, around one and two blocks, and
# around the tile
RAW_LENGTHS = [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 128, T - 1, T, T + 1, 2 * T + 56]


def _luma_of(nbytes):
    """(w, h) with w * h == nbytes, both even: 6 wide, else 2 wide (whichever has an even height)."""
    for w in (6, 2):
        if nbytes % w == 0 and (nbytes // w) % 2 == 0:
            return w, nbytes // w
    raise ValueError(nbytes)


# (w, h), the smallest at which padding, row gathering and tiling can each go wrong:
#   2x2       Y 4 bytes, chroma 1 byte                                8x8       Y exactly one block: the padding is a block of its own
#   6x10      Y 60 bytes: the length field spills into a second block 14x4      Y 56 bytes, the first length that spills
#   10x22, 14x16, 14x18, 16x16   chroma 55, 56, 63, 64 bytes          24x16, 66x34   rows that straddle blocks, odd 4-byte units
#   a luma of T - 4 bytes: its padding crosses a tile boundary        lumas of exactly T and T + 128 bytes at width 64
#   520x520   several tiles for all three components
SMALL = [(2, 2), (8, 8), (6, 10), (14, 4), (10, 22), (14, 16), (14, 18), (16, 16), (24, 16), (66, 34), _luma_of(T - 4), (64, T // 64), (64, (T + 128) // 64),
         (520, 520)]
assert all(w % 2 == 0 and h % 2 == 0 for w, h in SMALL) and SMALL[10][0] * SMALL[10][1] == T - 4
LARGE = (1920, 1088)
