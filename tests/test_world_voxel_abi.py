"""The world voxel filter's part of the C-ABI: the workspace size, the null-context refusal and the params helper (the layouts are
tests/test_abi_layout.py).  No GPU needed."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_workspace_bytes(built):
    f = built.load().prs_world_voxel_workspace_bytes
    # per sequence: 48 bytes a slot, 16 of drop counters, 4 a row (its slot) and 4 a chunk of 256 rows (its count); rounded up to 16
    formula = lambda B, N, T: (B * (48 * T + 16 + 4 * N + 4 * ((N + 255) // 256)) + 15) // 16 * 16  # noqa: E731
    assert f(1, 1, 1) == 80 and f(1, 256, 512) == formula(1, 256, 512) == 48 * 512 + 16 + 1024 + 4 + 12
    for shape in ((1, 257, 4), (3, 2305, 8192), (4096, 12288, 32768), (1, 443 * 4096, 1 << 22)):
        assert f(*shape) == formula(*shape) and f(*shape) % 16 == 0, shape
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert f(*bad) == 0


def test_null_context_is_refused(built):
    p, o = built.WorldVoxelParams(), built.WorldVoxelBatch()
    assert built.load().prs_world_voxel_batch_run(None, C.byref(p), C.byref(o)) == -1  # PRS_ERR_NULL


def test_params_helper(built):
    from srrg2_proslam_amd import ops
    p = ops.world_voxel_params(0.25)
    assert (p.voxel_size, p.position, list(p.reserved)) == (0.25, ops.VOXEL_REPRESENTATIVE, [0, 0])
    q = ops.world_voxel_params(2, position="mean")
    assert (q.voxel_size, q.position) == (2.0, ops.VOXEL_MEAN) and (ops.VOXEL_REPRESENTATIVE, ops.VOXEL_MEAN) == (0, 1)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):  # the last one is zero as a float32
        with pytest.raises(ValueError):
            ops.world_voxel_params(bad)
    with pytest.raises(ValueError):
        ops.world_voxel_params(0.1, position="median")
