"""The loop aligner's two entry points are exported and its structs have the header's layout (no GPU needed)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_point_align_entry_points_are_exported(built):
    lib = C.CDLL(built.LIB_PATH)
    for name in ("prs_point_align_batch", "prs_point_align"):
        assert hasattr(lib, name), name
    assert built.load().prs_version() == 104


def test_point_align_structs_have_the_header_layout(built):
    assert C.sizeof(built.PointAlignParams) == 11 * 4
    assert built.PointAlignParams.linearize_only.offset == 36
    # H, b, two chi sums, eight int32
    assert C.sizeof(built.PointAlignResult) == 36 * 4 + 6 * 4 + 2 * 4 + 8 * 4
    assert built.PointAlignResult.num_inliers.offset == 176 and built.PointAlignResult.warnings.offset == 204
    # four int32, ten pointers
    assert C.sizeof(built.PointAlignPairs) == 16 + 10 * 8
    assert built.PointAlignPairs.fixed.offset == 16 and built.PointAlignPairs.inlier_mask.offset == 16 + 9 * 8
