"""The depth consistency filter's part of the C-ABI: what the header says it leaves out, the workspace size, the null-context refusal
and the params helper (the layouts are tests/test_abi_layout.py).  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_header_says_what_the_stage_leaves_out():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "proslam_hip.h")).read()
    section = header[header.index(" * Depth consistency filter:"):header.index("} prs_depth_consistency_params;")]
    for left_out in ("a fused (averaged) depth", "a back-projection pixel-error test", "per-frame intrinsics", "bilinear", "a companion image",
                     "a host-pointer"):
        assert left_out in section, left_out


def test_workspace_bytes(built):
    f = built.load().prs_depth_consistency_workspace_bytes
    formula = lambda B, F, w: 64 * B * F * 2 * w  # a 64-byte record per image and slot  # noqa: E731
    assert f(1, 1, 1) == 128 and f(1, 5, 2) == 1280
    for shape in ((1, 1, 1), (3, 17, 8), (64, 16, 2), (256, 4, 4), (1, 64, 1), (2 ** 31 - 1, 1, 1), (1, 2 ** 31 - 1, 8), (2 ** 15, 2 ** 15, 8)):
        assert f(*shape) == formula(*shape) and f(*shape) % 16 == 0, shape
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1, -3, 2), (1, 1, -1), (1, 1, 9), (4, 4, 100), (2 ** 16, 2 ** 15, 1),
                (2 ** 31 - 1, 2 ** 31 - 1, 1)):
        assert f(*bad) == 0, bad


def test_null_context_is_refused(built):
    p, o = built.DepthConsistencyParams(), built.DepthConsistencyBatch()
    assert built.load().prs_depth_consistency_batch_run(None, C.byref(p), C.byref(o)) == -1  # PRS_ERR_NULL


def test_params_helper_and_batch_class(built):
    from srrg2_proslam_amd import configs, ops
    assert callable(ops.DepthConsistencyBatch)
    assert ops.DepthConsistencyBatch.OUTPUTS == ("support", "violation", "n_kept", "n_removed", "n_skipped")
    cam = dict(fx=481.2, fy=-480.0, cx=319.5, cy=239.5)
    p = ops.depth_consistency_params(cam)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    assert (p.window, p.stride, p.max_rel_diff, p.min_support, p.max_violation) == (2, 1, f32(0.02), 2, 1)
    assert (p.range_min, p.range_max, p.depth_type, p.depth_scaling_factor_to_meters) == (f32(0.1), 10.0, ops.DEPTH_U16, 1.0)
    assert (p.fx, p.fy, p.cx, p.cy) == (f32(481.2), -480.0, 319.5, 239.5)
    assert list(p.sensor_in_robot) == list(np.eye(4).reshape(16)) and list(p.reserved) == [0] * 3
    assert configs.DEPTH_CONSISTENCY == dict(window=2, stride=1, max_rel_diff=0.02, min_support=2, max_violation=1, range_min=0.1,
                                             range_max=10.0)
    q = ops.depth_consistency_params(cam, **configs.DEPTH_CONSISTENCY)
    assert bytes(q) == bytes(p)
    S = np.arange(16, dtype=np.float32).reshape(4, 4)
    q = ops.depth_consistency_params(cam, 8, 3, 0.0, 0, 16, 0.0, 0.0, "f32", 1e-3, S)
    assert (q.window, q.stride, q.max_rel_diff, q.min_support, q.max_violation, q.range_min, q.range_max) == (8, 3, 0.0, 0, 16, 0.0, 0.0)
    assert (q.depth_type, q.depth_scaling_factor_to_meters, list(q.sensor_in_robot)) == (ops.DEPTH_F32, f32(1e-3), list(range(16)))
    nan, inf = float("nan"), float("inf")
    for bad in (dict(window=0), dict(window=9), dict(window=1.5), dict(stride=0), dict(stride=2 ** 31), dict(min_support=-1),
                dict(min_support=17), dict(max_violation=-1), dict(max_violation=17), dict(max_rel_diff=-1e-9), dict(max_rel_diff=nan),
                dict(max_rel_diff=inf), dict(max_rel_diff=1e39), dict(depth_type="u8"), dict(depth_type=2), dict(scale=0.0),
                dict(scale=-1.0), dict(scale=nan), dict(range_min=-0.1), dict(range_min=2.0, range_max=1.0), dict(range_max=inf),
                dict(sensor_in_robot=np.full((4, 4), nan))):
        with pytest.raises(ValueError):
            ops.depth_consistency_params(cam, **bad)
    with pytest.raises(ValueError):
        ops.depth_consistency_params(dict(cam, fx=nan))
