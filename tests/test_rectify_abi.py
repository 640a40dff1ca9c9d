"""The image rectifier's null-context refusal and its Python helpers (the layouts are tests/test_abi_layout.py; no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

K = np.array([[458.654, 0.0, 367.215], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]])
DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_null_context_is_refused(built):
    p, b = built.RectifyParams(), built.RectifyBatch()
    assert built.load().prs_rectify_batch_run(None, C.byref(p), C.byref(b)) == -1
    assert built.load().prs_rectify_batch_run(None, None, None) == -1


def test_rectify_params_defaults_and_refusals(built):
    from srrg2_proslam_amd import ops
    p = ops.rectify_params()
    assert (p.pixel_type, p.interpolation, p.border, p.reserved) == (ops.PIXEL_U8, ops.RECTIFY_BILINEAR, 0.0, 0)
    assert ops.rectify_params("u16").interpolation == ops.RECTIFY_NEAREST
    assert ops.rectify_params("f32").interpolation == ops.RECTIFY_NEAREST
    assert ops.rectify_params("u8", "nearest", 255).border == 255.0
    assert ops.rectify_params("u16", border=65535).border == 65535.0
    assert np.isnan(ops.rectify_params("f32", border=float("nan")).border)
    for bad in (dict(pixel_type="u32"), dict(pixel_type="u16", interpolation="bilinear"), dict(pixel_type="f32", interpolation="bilinear"),
                dict(interpolation="cubic"), dict(border=256), dict(border=-1), dict(pixel_type="u16", border=65536),
                dict(border=float("nan"))):
        with pytest.raises(ValueError):
            ops.rectify_params(**bad)


def test_rectify_map_validates(built):
    from srrg2_proslam_amd import ops
    m = ops.rectify_map(K, DIST[:4])
    s = m.struct()
    assert (s.model, s.k3, s.src_fx, s.dst_cy) == (0, 0.0, np.float32(458.654), np.float32(248.375))
    assert list(s.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    bad_k = K.copy()
    bad_k[0, 0] = 0.0
    nan_k = K.copy()
    nan_k[1, 2] = np.nan
    big_k = K.copy()
    big_k[0, 2] = 1e300  # finite as a float64, not as the float32 the kernel is handed
    for args in ((bad_k, DIST), (nan_k, DIST), (big_k, DIST), (K[:2], DIST), (K, DIST[:3]), (K, (np.inf, 0, 0, 0, 0)),
                 (K, DIST, np.zeros((3, 3))), (K, DIST, np.full((3, 3), np.nan)), (K, DIST, np.eye(4)), (K, DIST, np.eye(3), bad_k)):
        with pytest.raises(ValueError):
            ops.rectify_map(*args)
    with pytest.raises(ValueError):
        ops.stereo_rectification(K, DIST, K, DIST, np.eye(3), [0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        ops.stereo_rectification(K, DIST, K, DIST, np.eye(3), [0.0, 0.0, 0.1])  # no row can be shared along the optical axis
