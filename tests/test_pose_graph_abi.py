"""The pose-graph optimiser's entry points are exported and its structs have the layout the library was compiled with (no GPU needed)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_pose_graph_entry_points_are_exported(built):
    lib = C.CDLL(built.LIB_PATH)
    for name in ("prs_pose_graph_workspace_bytes", "prs_pose_graph_struct_sizes", "prs_pose_graph_optimize_batch",
                 "prs_pose_graph_append_closures", "prs_pose_graph_optimize"):
        assert hasattr(lib, name), name
    assert built.load().prs_version() == 104  # new entries under the current version, prs_abi_check unchanged
    assert built.load().prs_status_string(built.ERR_NOT_POSITIVE_DEFINITE) != built.load().prs_status_string(-99)


def test_pose_graph_structs_have_the_library_layout(built):
    sizes = (C.c_uint64 * 4)()
    built.load().prs_pose_graph_struct_sizes(sizes)
    mine = [C.sizeof(t) for t in (built.PoseGraphParams, built.PoseGraphResult, built.PoseGraphs, built.PoseGraphClosures)]
    assert list(sizes) == mine
    assert mine == [5 * 4, 32 * 8 + 8 + 4 * 4, 16 + 10 * 8 + 8, 16 + 8 * 8]
    assert built.PoseGraphResult.chi_final.offset == 256 and built.PoseGraphResult.status.offset == 276
    assert built.PoseGraphs.X.offset == 16 and built.PoseGraphs.workspace_bytes.offset == 16 + 9 * 8 and built.PoseGraphs.result.offset == 96


def test_workspace_bytes(built):
    f = built.load().prs_pose_graph_workspace_bytes
    assert f(1, 114, 1064) == 1064 * 288 and f(64, 455, 21967) == 64 * 21967 * 288 and f(0, 8, 8) == 0
