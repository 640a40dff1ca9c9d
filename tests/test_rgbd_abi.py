"""The library exports the RGB-D preprocessor's two entry points and reports the ABI version that adds them (no GPU needed)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_rgbd_entry_points_are_exported(built):
    lib = C.CDLL(built.LIB_PATH)
    for name in ("prs_depth_measurements_batch", "prs_depth_measurements"):
        assert hasattr(lib, name), name
    assert built.load().prs_version() == 104


def test_rgbd_structs_have_the_header_layout(built):
    assert C.sizeof(built.DepthParams) == 8
    # 4 ints, depth, stride (padded), 6 input pointers, 5 output pointers
    assert C.sizeof(built.DepthBatch) == 16 + 8 + 8 + 10 * 8
    assert built.DepthBatch.fixed.offset == 16 + 8 + 8 + 5 * 8
