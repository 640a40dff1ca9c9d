"""The dense RGB-D cloud's part of the C-ABI: the workspace size, the null-context refusal and the params helper (the layouts are
tests/test_abi_layout.py).  No GPU needed."""
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
