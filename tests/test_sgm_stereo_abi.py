"""Semi-global dense stereo's part of the C-ABI: its batch against dense stereo's, the workspace size with its volume term, the
null-context refusal and the params helper (the layouts are tests/test_abi_layout.py).  No GPU needed."""
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


def test_batch_is_the_dense_stereo_batch_with_images_in_flight(built):
    """the fields of prs_dense_stereo_batch, with images_in_flight in the place of reserved0"""
    B, D = built.SgmStereoBatch, built.DenseStereoBatch
    assert [(n, getattr(B, n).offset) for n, _ in B._fields_ if n != "images_in_flight"] == \
        [(n, getattr(D, n).offset) for n, _ in D._fields_ if n != "reserved0"]
    assert B.images_in_flight.offset == D.reserved0.offset


def test_workspace_bytes(built):
    f = built.load().prs_sgm_stereo_workspace_bytes
    up = lambda x: (x + 15) // 16 * 16  # noqa: E731

    def formula(B, F, r, c, n, lr, k):
        """two census images and the left records, 8 bytes a pixel each; the right winners, 2 bytes a pixel; one uint16 volume for the
        images in flight"""
        P, Q = B * F * r * c, min(k, B * F) * r * c * n
        return 3 * up(8 * P) + (up(2 * P) if lr else 0) + up(2 * Q)

    assert f(1, 1, 1, 1, 1, 0, 1) == 48 + 16 and f(1, 1, 1, 1, 1, 1, 1) == 64 + 16
    assert f(1, 1, 376, 1241, 128, 1, 1) == (3 * 8 + 2 + 2 * 128) * 376 * 1241
    shapes = ((1, 1, 3, 5, 16, 1, 1), (3, 2, 17, 65, 37, 0, 4), (3, 2, 17, 65, 37, 0, 6), (3, 2, 17, 65, 37, 1, 7), (3, 2, 17, 65, 37, 1, 1 << 30),
              (2, 5, 9, 13, 1, 7, 3), (1, 4, 376, 1241, 128, 0, 2), (1024, 1, 376, 1241, 128, 1, 8),
              (64, 1, 480, 752, 256, 1, 64), (64, 1, 480, 752, 256, 1, 100))  # the last two: Q = 5.9e9 elements, beyond 2^31 and 2^32
    for shape in shapes:
        assert f(*shape) == formula(*shape) and f(*shape) % 16 == 0, shape
    assert 64 * 480 * 752 * 256 > 1 << 32 and f(*shapes[-1]) == f(*shapes[-2]) > 2 * (1 << 32)
    assert f(3, 2, 17, 65, 37, 0, 6) == f(3, 2, 17, 65, 37, 0, 1000) > f(3, 2, 17, 65, 37, 0, 5)
    for bad in ((0, 1, 1, 1, 1, 1, 1), (1, 0, 1, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1, 1), (1, 1, 1, 0, 1, 1, 1), (1, 1, 1, 1, 0, 1, 1),
                (1, 1, 1, 1, 257, 1, 1), (1, 1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 1, 1, -3), (-1, 1, 1, 1, 1, 1, 1), (1, 1, 1 << 16, 1 << 16, 16, 1, 1),
                (1, 1 << 12, 1 << 10, 1 << 10, 16, 0, 1), (1 << 20, 1 << 20, 1, 1, 16, 0, 1)):
        assert f(*bad) == 0, bad


def test_null_context_is_refused(built):
    p, o = built.SgmStereoParams(), built.SgmStereoBatch()
    assert built.load().prs_sgm_stereo_batch_run(None, C.byref(p), C.byref(o)) == -1  # PRS_ERR_NULL


def test_params_helper_and_batch_class(built):
    from srrg2_proslam_amd import configs, ops
    assert callable(ops.SgmStereoBatch) and ops.SgmStereoBatch.OUTPUTS == ("disparity", "depth", "n_valid")
    assert configs.SGM_STEREO == dict(n_disparities=128, min_disparity=0, p1=10, p2=120, n_paths=8, uniqueness_percent=10, lr_max_diff=1)
    assert isinstance(configs.SGM_STEREO_VOLUME_BUDGET, int) and configs.SGM_STEREO_VOLUME_BUDGET >= 2 * 376 * 1241 * 256
    # images_in_flight when it is left to the batch class: the volumes of 8 KITTI images at 256 disparities, of 17 at 128, stay within
    # the budget; at least 1, at most the images of the batch
    budget = configs.SGM_STEREO_VOLUME_BUDGET
    for n, batch in ((256, 1024), (128, 1024), (128, 5), (256, 1)):
        k = ops.sgm_stereo_images_in_flight(batch, 1, 376, 1241, n)
        volume = 2 * 376 * 1241 * n
        assert k == min(batch, budget // volume) and k * volume <= budget and (k == batch or (k + 1) * volume > budget), (n, batch)
    assert ops.sgm_stereo_images_in_flight(4, 2, 1 << 13, 1 << 13, 256) == 1  # one volume alone passes the budget
    p = ops.sgm_stereo_params(KITTI)
    assert (p.n_disparities, p.min_disparity, p.p1, p.p2, p.n_paths, p.uniqueness_percent, p.lr_max_diff, list(p.reserved)) == \
        (128, 0, 10, 120, 8, 10, 1, [0] * 4)
    assert p.bf == float(np.float32(np.float64(718.856) * np.float64(0.537166)))
    assert ops.sgm_stereo_params(configs.KITTI["camera"]).bf == p.bf
    q = ops.sgm_stereo_params(KITTI, 256, 3840, 4095, 4095, 4, 99, 255)
    assert (q.n_disparities, q.min_disparity, q.p1, q.p2, q.n_paths, q.uniqueness_percent, q.lr_max_diff) == (256, 3840, 4095, 4095, 4, 99, 255)
    q = ops.sgm_stereo_params(KITTI, 1, 0, 0, 0, 8, 0, -1)
    assert (q.n_disparities, q.p1, q.p2, q.uniqueness_percent, q.lr_max_diff) == (1, 0, 0, 0, -1)
    for bad in (dict(n_disparities=0), dict(n_disparities=257), dict(min_disparity=-1), dict(min_disparity=3969), dict(p1=-1), dict(p1=121),
                dict(p2=9), dict(p2=4096), dict(p1=4096, p2=4096), dict(n_paths=0), dict(n_paths=2), dict(n_paths=5), dict(n_paths=16),
                dict(uniqueness_percent=-1), dict(uniqueness_percent=100), dict(lr_max_diff=-2), dict(lr_max_diff=256)):
        with pytest.raises(ValueError):
            ops.sgm_stereo_params(KITTI, **bad)
    for cam in (dict(KITTI, baseline_m=0.0), dict(KITTI, fx=-700.0), dict(KITTI, fx=float("nan")), dict(KITTI, fx=float("inf")),
                dict(KITTI, fx=1e30, baseline_m=1e30), dict(KITTI, baseline_m=1e-60)):
        with pytest.raises(ValueError):
            ops.sgm_stereo_params(cam)
