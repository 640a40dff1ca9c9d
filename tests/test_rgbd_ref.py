"""The CPU checker of the RGB-D preprocessor (tests/rgbd_ref.py) against the ICL fixture's own depth lookup
(tests/ref_pins.py::icl_measurements, fixtures.hpp:565-650) and on hand cases for the rounding and depth-value edges."""
import numpy as np
import pytest

import ref_pins as rp
import rgbd_ref as rr
from test_ref_pins import OracleBackend


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("k", [0, 1, 50])
def test_checker_reproduces_the_icl_fixture(k):
    B = OracleBackend()
    uv, desc, inten = B.extract(rp.icl_gray(k), 5, 500, 3, 3)
    ref = rp.icl_measurements(B, k)
    uvd, d, i, status = rr.measurements(rp.icl_depth_m(k), uv, desc, 1.0, inten)
    assert np.array_equal(_bits(uvd[:, :2]), _bits(ref["uv"]))
    assert np.array_equal(_bits(uvd[:, 2]), _bits(ref["depth"]))
    assert np.array_equal(d, ref["desc"]) and np.array_equal(_bits(i), _bits(ref["intensity"]))
    assert len(uvd) > 200 and status in (0, rr.WARN_SPARSE_DEPTH)
    # the uint16 millimetre image with scale 0.001f gives the same bits as the float metre image with scale 1
    mm = rp.load("ref_icl")["depth_mm"][{0: 0, 1: 1, 50: 2}[k]]
    assert mm.dtype == np.uint16
    uvd16, d16, i16, status16 = rr.measurements(mm, uv, desc, np.float32(1e-3), inten)
    assert np.array_equal(_bits(uvd16), _bits(uvd)) and np.array_equal(d16, d) and status16 == status


def test_rounding_is_half_to_even():
    depth = np.arange(1, 1 + 6 * 7, dtype=np.float32).reshape(6, 7)
    kp = np.array([[2.5, 0.0], [3.5, 0.0], [-0.5, -0.5], [0.0, 2.5], [0.0, 3.5], [6.49, 5.5 - 1.0], [1.4999999, 1.5000001]], np.float32)
    idx, d, status = rr.read_depth(depth, kp, 1.0)
    assert list(idx) == list(range(7)) and status == 0
    # (row, col): (0, 2), (0, 4), (0, 0), (2, 0), (4, 0), (4, 6), (2, 1)
    expect = [depth[0, 2], depth[0, 4], depth[0, 0], depth[2, 0], depth[4, 0], depth[4, 6], depth[2, 1]]
    assert np.array_equal(d, np.array(expect, np.float32))


@pytest.mark.parametrize("u,v", [(-0.51, 0.0), (0.0, -0.51), (6.5, 0.0), (0.0, 5.5), (np.nan, 0.0), (0.0, np.inf)])
def test_outside_the_image_is_a_range_error(u, v):
    depth = np.ones((6, 7), np.float32)  # cols 7 (odd): 6.5 rounds to 6 (inside); rows 6 (even): 5.5 rounds to 6 (outside)
    kp = np.array([[1.0, 1.0], [u, v]], np.float32)
    expect_inside = (u, v) == (6.5, 0.0)
    idx, _, status = rr.read_depth(depth, kp, 1.0)
    if expect_inside:
        assert status == 0 and list(idx) == [0, 1]
    else:
        assert idx is None and status == rr.ERR_RANGE


def test_depth_value_edges():
    tiny = np.float32(np.finfo(np.float32).smallest_subnormal)
    vals = np.array([0.0, -0.0, -1.0, np.nan, np.inf, tiny, 2.0, 1e-3], np.float32)
    depth = vals[None, :]
    kp = np.stack([np.arange(len(vals), dtype=np.float32), np.zeros(len(vals), np.float32)], axis=1)
    idx, d, status = rr.read_depth(depth, kp, np.float32(1e-3))
    assert list(idx) == [4, 5, 6, 7]
    assert np.isposinf(d[0]) and _bits(d[1]) == 0  # a positive denormal is kept even when the scaled depth underflows to 0
    assert d[2] == np.float32(2.0) * np.float32(1e-3) and d[3] == np.float32(1e-3) * np.float32(1e-3)
    assert status == rr.WARN_SPARSE_DEPTH  # 4 of 8 without depth
    u16 = np.array([[0, 1, 65535]], np.uint16)
    idx, d, _ = rr.read_depth(u16, [[0, 0], [1, 0], [2, 0]], 1.0)
    assert list(idx) == [1, 2] and list(d) == [1.0, 65535.0]


def test_status_rules():
    depth = np.ones((4, 8), np.uint16)
    kp = np.stack([np.arange(8, dtype=np.float32), np.zeros(8, np.float32)], axis=1)
    for holes, expect in [(0, 0), (2, 0), (3, rr.WARN_SPARSE_DEPTH), (8, rr.WARN_NO_MATCHES)]:
        d = depth.copy()
        d[0, :holes] = 0
        assert rr.read_depth(d, kp, 1.0)[2] == expect, holes  # 2 / 8 = 0.25 exactly: no warning
    assert rr.read_depth(depth, kp[:0], 1.0)[2] == rr.WARN_NO_MATCHES
    assert rr.read_depth(depth, kp, 1.0, n_features=8, stride=7)[2] == rr.ERR_CAPACITY
    assert rr.read_depth(depth, kp, 1.0, extract_status=-2)[2] == -2
    # the ratio is a float32 division: 4097 / 16385 rounds to 0.25000763, above; n = 2^25 + 4 and 2^23 + 1 without depth
    # rounds the quotient to 0.25 exactly, not above
    assert np.float32(4097) / np.float32(16385) > 0.25
    assert not np.float32(2 ** 23 + 1) / np.float32(2 ** 25 + 4) > 0.25
