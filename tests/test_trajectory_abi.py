"""The trajectory evaluator's part of the C-ABI: the null-context refusal and the params helper (the layouts, the result's numpy
dtype among them, are tests/test_abi_layout.py).  No GPU needed."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


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
