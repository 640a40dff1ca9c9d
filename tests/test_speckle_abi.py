"""The speckle filter's part of the C-ABI: the header's pointer to it, the workspace size, the null-context refusal and the params
helper (the layouts are tests/test_abi_layout.py).  No GPU needed."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_dense_stereo_section_points_to_the_filter():
    """dense stereo no longer lists the filter among what it left out"""
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "proslam_hip.h")).read()
    dense = header[header.index(" * Dense stereo:"):header.index("} prs_dense_stereo_params;")]
    assert "a speckle filter," not in dense and "prs_speckle_batch_run" in dense


def test_workspace_bytes(built):
    f = built.load().prs_speckle_workspace_bytes
    up = lambda x: (x + 15) // 16 * 16  # noqa: E731
    formula = lambda B, F, r, c: 2 * up(4 * B * F * r * c)  # a parent and a size, int32, per pixel  # noqa: E731
    assert f(1, 1, 1, 1) == 32 and f(1, 1, 1, 5) == 64 and f(1, 1, 2, 2) == 32
    assert f(1, 1, 376, 1241) == 2 * 4 * 376 * 1241
    for shape in ((1, 1, 3, 5), (3, 2, 17, 65), (64, 1, 480, 752), (2, 5, 9, 13), (1024, 1, 376, 1241), (1, 1, 1, 2 ** 31 - 1)):
        assert f(*shape) == formula(*shape) and f(*shape) % 16 == 0, shape
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-1, 1, 1, 1), (1, 1, 1, -5), (1, 1, 1 << 16, 1 << 15),
                (1, 1 << 12, 1 << 10, 1 << 10), (1 << 20, 1 << 20, 1, 1), (2, 1, 1, 1 << 30)):
        assert f(*bad) == 0, bad


def test_null_context_is_refused(built):
    p, o = built.SpeckleParams(), built.SpeckleBatch()
    assert built.load().prs_speckle_batch_run(None, C.byref(p), C.byref(o)) == -1  # PRS_ERR_NULL


def test_params_helper_and_batch_class(built):
    from srrg2_proslam_amd import configs, ops
    assert callable(ops.SpeckleFilterBatch) and ops.SpeckleFilterBatch.OUTPUTS == ("label", "n_kept", "n_removed")
    p = ops.speckle_params()
    assert (p.max_size, p.max_diff, p.pixel_type, p.companion_type, list(p.reserved)) == (200, 1.0, ops.PIXEL_F32, ops.PIXEL_F32, [0] * 4)
    assert configs.SPECKLE == dict(max_size=200, max_diff=1.0)
    q = ops.speckle_params(**configs.SPECKLE)
    assert (q.max_size, q.max_diff) == (p.max_size, p.max_diff)
    q = ops.speckle_params(2 ** 31 - 1, 3e38, "u16")
    assert (q.max_size, q.max_diff, q.pixel_type, q.companion_type) == (2 ** 31 - 1, float(np.float32(3e38)), ops.PIXEL_U16, ops.PIXEL_U16)
    q = ops.speckle_params(0, 0.0, "f32", "u16")
    assert (q.max_size, q.max_diff, q.pixel_type, q.companion_type) == (0, 0.0, ops.PIXEL_F32, ops.PIXEL_U16)
    assert ops.speckle_params(max_diff=0.1).max_diff == float(np.float32(0.1))
    for bad in (dict(max_size=-1), dict(max_size=2 ** 31), dict(max_size=1.5), dict(max_diff=-1e-9), dict(max_diff=float("nan")),
                dict(max_diff=float("inf")), dict(max_diff=1e39), dict(pixel_type="u8"), dict(pixel_type="f64"), dict(pixel_type=2),
                dict(companion_type="u8"), dict(companion_type="rgb")):
        with pytest.raises(ValueError):
            ops.speckle_params(**bad)
