"""The 16-byte entry of the search kernel's query cache (AlignArgs::qcache in csrc/align.hip), restated in numpy from the header
comment there and packed / unpacked over every corner value.  No device is needed.

    x = cx0 | cx1 << 8 | cy0 << 16 | cy1 << 24                 the cell rectangle the scan covered, one byte each
    s_i = lattice position (11 bits) | full distance << 11 (9 bits: 0 .. 256), up to four distinct survivors
    y = s_0 | (survivors + 1) << 20                            three bits; 0 = invalid (an invalid entry is all zero)
    z = s_1 | position of s_3 << 20
    w = s_2 | distance of s_3 << 20
"""
import itertools

import numpy as np

POSITION_BITS, DISTANCE_BITS = 11, 9


def pack(rect, survivors):
    """rect: (cx0, cx1, cy0, cy1); survivors: up to four (position, distance) -> uint32[4]"""
    assert len(survivors) <= 4
    e = np.zeros(4, np.uint32)
    e[0] = rect[0] | rect[1] << 8 | rect[2] << 16 | rect[3] << 24
    s = [p | d << POSITION_BITS for p, d in survivors]
    e[1] = (s[0] if len(s) > 0 else 0) | (len(s) + 1) << 20
    e[2] = (s[1] if len(s) > 1 else 0) | (survivors[3][0] << 20 if len(s) > 3 else 0)
    e[3] = (s[2] if len(s) > 2 else 0) | (survivors[3][1] << 20 if len(s) > 3 else 0)
    return e


def unpack(e):
    """uint32[4] -> (rect, survivors), or None for an invalid entry; every field a shift and a mask"""
    x, y, z, w = (int(v) for v in e)
    code = y >> 20
    if code == 0:
        return None
    words = (y, z, w)
    survivors = [(words[i] & 0x7ff, (words[i] >> 11) & 0x1ff) for i in range(min(code - 1, 3))]
    if code - 1 == 4:
        survivors.append(((z >> 20) & 0x7ff, w >> 20))
    return (x & 0xff, (x >> 8) & 0xff, (x >> 16) & 0xff, x >> 24), survivors


def test_an_invalid_entry_is_all_zero_and_no_valid_entry_is():
    assert unpack(np.zeros(4, np.uint32)) is None
    for n in range(5):
        e = pack((0, 0, 0, 0), [(0, 0)] * n)
        assert e[1] != 0 and unpack(e) == ((0, 0, 0, 0), [(0, 0)] * n)


def test_every_corner_value_survives_a_round_trip():
    corners = [(p, d) for p in (0, 1, 1023, 1024, 2047) for d in (0, 1, 255, 256)]
    rects = [(0, 0, 0, 0), (255, 255, 255, 255), (0, 255, 0, 255), (1, 2, 3, 4), (77, 78, 22, 23)]
    seen = 0
    for n in range(5):
        for survivors in itertools.product(corners, repeat=n):
            if n == 4 and (seen % 7):  # (all 160 000 four-survivor combinations are not needed: every seventh, and all below)
                seen += 1
                continue
            seen += 1
            for rect in rects[:2] if n > 2 else rects:
                e = pack(rect, list(survivors))
                assert e.dtype == np.uint32
                assert unpack(e) == (rect, list(survivors))
    # every field at its largest value at once, and each alone: no field reaches into a neighbour
    full = [(2047, 256)] * 4
    assert unpack(pack((255, 255, 255, 255), full)) == ((255, 255, 255, 255), full)
    for i in range(4):
        for p, d in ((2047, 0), (0, 256)):
            one = [(0, 0)] * 4
            one[i] = (p, d)
            assert unpack(pack((0, 0, 0, 0), one)) == ((0, 0, 0, 0), one)


def test_the_rectangle_bytes_are_where_they_were():
    e = pack((0x12, 0x34, 0x56, 0x78), [(2047, 256)] * 4)
    assert int(e[0]) == 0x78563412
    assert e.view(np.uint8)[:4].tolist() == [0x12, 0x34, 0x56, 0x78]  # (little-endian: cx0, cx1, cy0, cy1)


def test_the_fields_fit_what_the_kernel_can_meet():
    # a lattice position is at most max_fixed (the sentinel behind the last entry), and the plan refuses max_fixed >= 2048;
    # a 256-bit Hamming distance is at most 256; the count code is survivors + 1 <= 5
    assert 2047 < 1 << POSITION_BITS and 256 < 1 << DISTANCE_BITS and 5 < 1 << 3
    assert POSITION_BITS + DISTANCE_BITS == 20 and 20 + 3 <= 32 and 20 + 11 <= 32 and 20 + 9 <= 32
