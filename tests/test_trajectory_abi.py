"""The trajectory evaluator's part of the C-ABI: entry points exported, struct layouts agreed between the library, the header's
declared sizes and the ctypes mirrors, and the ABI version unchanged (new entries under the current version).  No GPU needed."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_entry_points_exported(built):
    lib = C.CDLL(built.LIB_PATH)
    for name in ("prs_trajectory_eval_batch", "prs_trajectory_struct_sizes"):
        assert hasattr(lib, name), name
        assert name in built.SYMBOLS


def test_struct_sizes_match_the_library(built):
    lib = built.load()
    sizes = (C.c_uint64 * 3)()
    lib.prs_trajectory_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(built.TrajectoryParams), C.sizeof(built.TrajectoryResult), C.sizeof(built.TrajectoryBatch)]
    # as the header lays them out: 4 int32 + 8 float; 4 int32 + 56 double + 8 int32; 2 int32 + 7 pointers
    assert list(sizes) == [48, 496, 64]
    assert built.TrajectoryResult.S.offset == 16 and built.TrajectoryResult.kitti_n_len.offset == 464
    from srrg2_proslam_amd import ops
    assert ops._TRAJ_RESULT_DTYPE.itemsize == 496
    for name, _ in built.TrajectoryResult._fields_:
        assert ops._TRAJ_RESULT_DTYPE.fields[name][1] == getattr(built.TrajectoryResult, name).offset, name


def test_version_unchanged(built):
    assert built.load().prs_version() == 104 == built.ABI_VERSION


def test_null_context_is_refused(built):
    p, b = built.TrajectoryParams(), built.TrajectoryBatch()
    assert built.load().prs_trajectory_eval_batch(None, C.byref(p), C.byref(b)) == -1  # PRS_ERR_NULL


def test_params_helper(built):
    from srrg2_proslam_amd import ops
    p = ops.trajectory_params()
    assert (p.align, p.rpe_delta, p.kitti_step, p.n_lengths) == (built.TRAJ_ALIGN_RIGID, 1, 10, 8)
    assert list(p.lengths) == [100, 200, 300, 400, 500, 600, 700, 800]
    q = ops.trajectory_params(align="first", rpe_delta=7, kitti_step=0, lengths=(5, 10))
    assert (q.align, q.rpe_delta, q.kitti_step, q.n_lengths) == (built.TRAJ_ALIGN_FIRST, 7, 0, 2)
    with pytest.raises(ValueError):
        ops.trajectory_params(lengths=range(1, 10))
