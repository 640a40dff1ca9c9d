"""The world voxel filter's part of the C-ABI: entry points exported, struct layouts agreed between the library, the header's declared
sizes and the ctypes mirrors, the workspace size, the params helper, and the ABI version unchanged (new entries under the current
version).  No GPU needed."""
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
    for name in ("prs_world_voxel_batch_run", "prs_world_voxel_workspace_bytes", "prs_world_voxel_struct_sizes"):
        assert hasattr(lib, name), name
        assert name in built.SYMBOLS


def test_struct_sizes_and_offsets_match_the_library(built):
    lib = built.load()
    sizes = (C.c_uint64 * 2)()
    lib.prs_world_voxel_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(built.WorldVoxelParams), C.sizeof(built.WorldVoxelBatch)]
    # as the header lays them out: a float and three int32; 2 int32 + 6 pointers, 2 int32 + 13 pointers
    assert list(sizes) == [16, 168]
    P, B = built.WorldVoxelParams, built.WorldVoxelBatch
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("voxel_size", 0), ("position", 4), ("reserved", 8)]
    assert [n for n, _ in B._fields_] == ["batch", "in_stride", "in_xyz", "in_n", "in_n_opt", "in_desc", "in_node", "in_row", "out_stride",
                                          "table_stride", "xyz", "index", "count", "desc", "node", "row", "n_opt", "n_out", "n_voxels",
                                          "n_nonfinite", "n_outside", "status", "workspace"]
    assert [getattr(B, n).offset for n, _ in B._fields_] == [0, 4] + list(range(8, 56, 8)) + [56, 60] + list(range(64, 168, 8))


def test_workspace_bytes(built):
    f = built.load().prs_world_voxel_workspace_bytes
    # per sequence: 48 bytes a slot, 16 of drop counters, 4 a row (its slot) and 4 a chunk of 256 rows (its count); rounded up to 16
    formula = lambda B, N, T: (B * (48 * T + 16 + 4 * N + 4 * ((N + 255) // 256)) + 15) // 16 * 16  # noqa: E731
    assert f(1, 1, 1) == 80 and f(1, 256, 512) == formula(1, 256, 512) == 48 * 512 + 16 + 1024 + 4 + 12
    for shape in ((1, 257, 4), (3, 2305, 8192), (4096, 12288, 32768), (1, 443 * 4096, 1 << 22)):
        assert f(*shape) == formula(*shape) and f(*shape) % 16 == 0, shape
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert f(*bad) == 0


def test_version_unchanged(built):
    assert built.load().prs_version() == 104 == built.ABI_VERSION


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
