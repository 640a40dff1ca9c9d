"""Dense stereo's part of the C-ABI: the workspace size, the null-context refusal and the params helper (the layouts are
tests/test_abi_layout.py).  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

KITTI = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, baseline_m=0.537166)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_workspace_bytes(built):
    f = built.load().prs_dense_stereo_workspace_bytes
    up = lambda x: (x + 15) // 16 * 16  # noqa: E731
    # two census images and the left pass's records, 8 bytes a pixel each; the right pass's winners, 2 bytes a pixel
    formula = lambda B, F, r, c, n, lr: 3 * up(8 * B * F * r * c) + (up(2 * B * F * r * c) if lr else 0)  # noqa: E731
    assert f(1, 1, 1, 1, 1, 0) == 48 and f(1, 1, 1, 1, 1, 1) == 64
    assert f(1, 1, 376, 1241, 128, 1) == 3 * 8 * 376 * 1241 + 2 * 376 * 1241
    for shape in ((1, 1, 3, 5, 16, 1), (3, 2, 17, 65, 37, 0), (64, 1, 480, 752, 256, 1), (2, 5, 9, 13, 1, 7), (1, 4, 376, 1241, 128, 0)):
        assert f(*shape) == formula(*shape) and f(*shape) % 16 == 0, shape
    for bad in ((0, 1, 1, 1, 1, 1), (1, 0, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1), (1, 1, 1, 0, 1, 1), (1, 1, 1, 1, 0, 1), (1, 1, 1, 1, 257, 1),
                (-1, 1, 1, 1, 1, 1), (1, 1, 1 << 16, 1 << 16, 16, 1), (1, 1 << 12, 1 << 10, 1 << 10, 16, 0), (1 << 20, 1 << 20, 1, 1, 16, 0)):
        assert f(*bad) == 0, bad


def test_null_context_is_refused(built):
    p, o = built.DenseStereoParams(), built.DenseStereoBatch()
    assert built.load().prs_dense_stereo_batch_run(None, C.byref(p), C.byref(o)) == -1  # PRS_ERR_NULL


def test_params_helper_and_batch_class(built):
    from srrg2_proslam_amd import configs, ops
    assert callable(ops.DenseStereoBatch) and ops.DenseStereoBatch.OUTPUTS == ("disparity", "depth", "n_valid")
    p = ops.dense_stereo_params(KITTI)
    assert (p.n_disparities, p.min_disparity, p.aggregation_radius, p.uniqueness_percent, p.lr_max_diff, list(p.reserved)) == \
        (128, 0, 3, 10, 1, [0] * 6)
    assert p.bf == float(np.float32(np.float64(718.856) * np.float64(0.537166)))
    assert ops.dense_stereo_params(configs.KITTI["camera"]).bf == p.bf
    q = ops.dense_stereo_params(KITTI, 256, 3840, 7, 99, 255)
    assert (q.n_disparities, q.min_disparity, q.aggregation_radius, q.uniqueness_percent, q.lr_max_diff) == (256, 3840, 7, 99, 255)
    q = ops.dense_stereo_params(KITTI, 1, 0, 0, 0, -1)
    assert (q.n_disparities, q.aggregation_radius, q.uniqueness_percent, q.lr_max_diff) == (1, 0, 0, -1)
    for bad in (dict(n_disparities=0), dict(n_disparities=257), dict(min_disparity=-1), dict(min_disparity=3969), dict(aggregation_radius=-1),
                dict(aggregation_radius=8), dict(uniqueness_percent=-1), dict(uniqueness_percent=100), dict(lr_max_diff=-2),
                dict(lr_max_diff=256)):
        with pytest.raises(ValueError):
            ops.dense_stereo_params(KITTI, **bad)
    for cam in (dict(KITTI, baseline_m=0.0), dict(KITTI, fx=-700.0), dict(KITTI, fx=float("nan")), dict(KITTI, fx=float("inf")),
                dict(KITTI, fx=1e30, baseline_m=1e30), dict(KITTI, baseline_m=1e-60)):
        with pytest.raises(ValueError):
            ops.dense_stereo_params(cam)
