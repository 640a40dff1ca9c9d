"""The dense RGB-D cloud's part of the C-ABI: entry points exported and bound, struct layouts agreed between the library, the header's
declared sizes and the ctypes mirrors, the workspace size, the params helper, and the ABI version unchanged (new entries under the
current version).  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

K = dict(fx=481.2, fy=-481.0, cx=319.5, cy=239.5)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_entry_points_exported(built):
    lib = C.CDLL(built.LIB_PATH)
    for name in ("prs_depth_cloud_batch_run", "prs_depth_cloud_workspace_bytes", "prs_depth_cloud_struct_sizes"):
        assert hasattr(lib, name), name
        assert name in built.SYMBOLS


def test_struct_sizes_and_offsets_match_the_library(built):
    lib = built.load()
    sizes = (C.c_uint64 * 2)()
    lib.prs_depth_cloud_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(built.DepthCloudParams), C.sizeof(built.DepthCloudBatch)]
    # as the header lays them out: 9 words, 16 floats, 3 reserved words; 8 int32 and 14 pointers
    assert list(sizes) == [112, 144]
    P, B = built.DepthCloudParams, built.DepthCloudBatch
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("depth_type", 0), ("depth_scaling_factor_to_meters", 4), ("fx", 8), ("fy", 12), ("cx", 16), ("cy", 20), ("range_min", 24),
        ("range_max", 28), ("step", 32), ("sensor_in_robot", 36), ("reserved", 100)]
    assert [n for n, _ in B._fields_] == ["batch", "frames", "rows", "cols", "pitch", "gray_pitch", "pose_stride", "out_stride", "depth",
                                          "gray", "n_images", "pose", "frame_index", "n_base", "xyz", "frame", "pixel", "n_out", "n_total",
                                          "n_skipped", "status", "workspace"]
    assert [getattr(B, n).offset for n, _ in B._fields_] == list(range(0, 32, 4)) + list(range(32, 144, 8))


def test_header_declares_the_structs_in_that_order(built):
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "proslam_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} prs_depth_cloud_batch;", header).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == ["batch", "frames", "cols", "pitch", "gray_pitch", "pose_stride", "out_stride"] + \
        [n for n, _ in built.DepthCloudBatch._fields_][8:]  # "int32_t rows, cols;" declares two
    assert "rows, cols;" in body


def test_workspace_bytes(built):
    f = built.load().prs_depth_cloud_workspace_bytes
    # one count per chunk of 1024 sampled pixels of an image, rounded up to 16 bytes
    formula = lambda B, F, r, c, s: (4 * B * F * ((-(-r // s) * -(-c // s) + 1023) // 1024) + 15) // 16 * 16  # noqa: E731
    assert f(1, 1, 1, 1, 1) == 16 and f(1, 64, 480, 640, 1) == 4 * 64 * 300 and f(256, 4, 480, 640, 4) == formula(256, 4, 480, 640, 4)
    for shape in ((1, 1, 32, 32, 1), (1, 1, 25, 41, 1), (3, 7, 29, 37, 3), (64, 16, 480, 640, 1), (2, 5, 480, 640, 1000)):
        assert f(*shape) == formula(*shape) and f(*shape) % 16 == 0, shape
    for bad in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (-1, 1, 1, 1, 1), (1, 1, 1 << 16, 1 << 16, 1),
                (1, 1 << 12, 1 << 10, 1 << 10, 1)):
        assert f(*bad) == 0, bad


def test_version_unchanged(built):
    assert built.load().prs_version() == 104 == built.ABI_VERSION


def test_null_context_is_refused(built):
    p, o = built.DepthCloudParams(), built.DepthCloudBatch()
    assert built.load().prs_depth_cloud_batch_run(None, C.byref(p), C.byref(o)) == -1  # PRS_ERR_NULL


def test_params_helper_and_batch_class(built):
    from srrg2_proslam_amd import ops
    assert callable(ops.DepthCloudBatch) and ops.DepthCloudBatch.OPTIONAL == ("frame", "pixel")
    p = ops.depth_cloud_params(K)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    assert (p.depth_type, p.depth_scaling_factor_to_meters, p.step, list(p.reserved)) == (ops.DEPTH_U16, 1.0, 1, [0, 0, 0])
    assert (p.fx, p.fy, p.cx, p.cy) == (f32(481.2), -481.0, 319.5, 239.5) and (p.range_min, p.range_max) == (f32(0.1), 10.0)
    assert list(p.sensor_in_robot) == np.eye(4).reshape(16).tolist()
    S = np.arange(16, dtype=np.float64).reshape(4, 4)
    q = ops.depth_cloud_params(K, 0.0, 4.5, step=4, depth_type="f32", scale=1e-3, sensor_in_robot=S)
    assert (q.depth_type, q.step, q.range_min, q.range_max) == (ops.DEPTH_F32, 4, 0.0, 4.5)
    assert q.depth_scaling_factor_to_meters == f32(1e-3) and list(q.sensor_in_robot) == list(range(16))
    for bad in (dict(range_min=-0.5), dict(range_min=3.0, range_max=2.0), dict(range_max=float("inf")), dict(range_min=float("nan")),
                dict(step=0), dict(scale=0.0), dict(scale=-1.0), dict(scale=1e-60), dict(scale=float("nan")), dict(depth_type="u8"),
                dict(sensor_in_robot=np.full((4, 4), np.nan))):
        with pytest.raises(ValueError):
            ops.depth_cloud_params(K, **bad)
    with pytest.raises(ValueError):
        ops.depth_cloud_params(dict(K, fx=float("inf")))
