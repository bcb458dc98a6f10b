"""The brick skip structure's index arithmetic (tests/brick_twin.py) pinned to values derived by hand from the formulas of
hsk_dev.h and hsk_create: the shapes tests/test_gpu_bricks.py runs on the device, the one hsk_create refuses, and two cubes."""
import numpy as np
import pytest

import brick_twin as BT

# (X, Y, Z): bxn, byn, brick words, super-bricks, super_ok -- every one of them ends at bshift 3 (X or Y is 8 mod 16, or the
# field fits 1024 words)
TABLE = {
    (328, 40, 44): (41, 5, 40, 44, True),
    (512, 64, 52): (64, 8, 112, 64, True),
    (528, 16, 20): (66, 2, 16, 17, True),
    (264, 264, 264): (33, 33, 1124, 729, True),
    (1048, 1048, 12): (131, 131, 1076, 1089, False),
    (648, 648, 648): (81, 81, 16608, 9261, False),
}


@pytest.mark.parametrize("dims", list(TABLE))
def test_layout_table(dims):
    X, Y, Z = dims
    bxn, byn, words, supers, ok = TABLE[dims]
    L = BT.layout(X, Y, Z)
    assert L["bshift"] == 3
    assert (L["bxn"], L["byn"], L["words"], L["supers"], L["super_ok"]) == (bxn, byn, words, supers, ok)
    assert L["total_words"] == words + 32
    assert BT.super_dim(X, 3) == (bxn + 3) // 4


def test_layout_of_cubes():
    assert (BT.bshift_of(96, 96, 96), BT.flag_words(96, 96, 96, 3)) == (3, 56)
    assert (BT.bshift_of(512, 512, 512), BT.flag_words(512, 512, 512, 4)) == (4, 1024)
    assert BT.flag_words(512, 512, 512, 3) == 8192          # (why the edge grows)
    assert BT.bshift_of(1024, 1024, 1024) == 5 and BT.super_ok(1024, 1024, 1024, 5)
    # a slab: the stored planes count, rounded up to whole bricks
    assert BT.flag_words(328, 40, 23, 3) == 20 and BT.layout(328, 40, 23)["bzn"] == 3
    # the refused shape's staged field: above 64 KiB
    assert BT.flag_words_total(648, 648, 648, 3) * 4 == 66560


def test_row_span():
    # 328 x 40 x 44: rows of 41 bits; row r starts at bit 41 r
    assert BT.row_span(0, 0, 41, 5) == (0, 0)
    assert BT.row_span(0, 3, 41, 5) == (3, 27)              # 123 = 3 * 32 + 27: 27 + 41 > 64, a third word
    assert BT.row_span(1, 2, 41, 5) == (8, 31)              # 287
    assert BT.row_span(5, 4, 41, 5) == (37, 5)              # the last row: 1189, its bits end at 1229 in word 38
    assert BT.row_span(1, 0, 64, 8) == (16, 0)              # 512 x 64 x 52: every row is two whole words


def test_bits_of_a_crafted_volume():
    X, Y, Z = 328, 40, 44
    vol = np.zeros((Z, Y, X, 2), np.int16)
    vol[..., 0], vol[..., 1] = 16384, 1
    picks = [(0, 0, 0), (7, 7, 7), (43, 39, 327), (8, 31, 296), (40, 24, 320)]      # (z, y, x)
    for z, y, x in picks:
        vol[z, y, x, 0] = -16384
    b = BT.brick_bits(vol)
    assert b.shape == (6, 5, 41) and b.sum() == 4            # (the first two share brick 0)
    want = {(0, 0, 0), (5, 4, 40), (1, 3, 37), (5, 3, 40)}
    assert {tuple(int(v) for v in i) for i in np.argwhere(b)} == want
    f = BT.field(vol)
    assert len(f) == 72 and f.dtype == np.uint32
    bits = sorted((bz * 5 + by) * 41 + bx for bz, by, bx in want)
    assert sorted(int(w) * 32 + k for w in np.flatnonzero(f[:40]) for k in range(32) if (f[w] >> np.uint32(k)) & 1) == bits
    s = BT.super_bits(b)
    assert s.shape == (2, 2, 11) and {tuple(int(v) for v in i) for i in np.argwhere(s)} == {(0, 0, 0), (1, 1, 10), (0, 0, 9), (1, 0, 10)}
    sup = sorted((sz * 2 + sy) * 11 + sx for sz, sy, sx in [(0, 0, 0), (1, 1, 10), (0, 0, 9), (1, 0, 10)])
    assert sorted(int(w) * 32 + k for w in range(32) for k in range(32) if (f[40 + w] >> np.uint32(k)) & 1) == sup
    # row (1, 3): bit0 = 8 * 41 = 328 -> sh 8; row (5, 3): bit0 = 28 * 41 = 1148 -> sh 28, 28 + 41 > 64, brick 40 >= 36
    assert BT.third_word_bricks(b) == [(5, 3, 40)]
    assert BT.set_bits_beyond_word(b, 37) == 2 and BT.set_bits_beyond_word(b, 38) == 1


def test_no_super_bits_when_they_do_not_fit():
    X, Y, Z = 1048, 1048, 12
    vol = np.zeros((Z, Y, X, 2), np.int16)
    vol[11, 1047, 1047] = (-1, 1)
    f = BT.field(vol)
    assert len(f) == 1076 + 32 and not f[1076:].any()
    bit = (1 * 131 + 130) * 131 + 130
    assert np.flatnonzero(f).tolist() == [bit >> 5] and int(f[bit >> 5]) == 1 << (bit & 31)
