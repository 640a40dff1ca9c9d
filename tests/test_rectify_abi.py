"""The image rectifier's C-ABI surface and its Python helpers (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([[458.654, 0.0, 367.215], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]])
DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_entries_exported_and_bound(built):
    lib = C.CDLL(built.LIB_PATH)
    for name in ("prs_rectify_batch_run", "prs_rectify_struct_sizes"):
        assert hasattr(lib, name) and name in built.SYMBOLS
    header = open(os.path.join(ROOT, "include", "proslam_hip.h")).read()
    for name in ("prs_rectify_map", "prs_rectify_params", "prs_rectify_batch", "PRS_DISTORTION_RADTAN = 0", "PRS_PIXEL_U8 = 0",
                 "PRS_PIXEL_U16 = 1", "PRS_PIXEL_F32 = 2", "PRS_RECTIFY_BILINEAR = 0", "PRS_RECTIFY_NEAREST = 1"):
        assert name in header


def test_struct_sizes_and_map_layout(built):
    lib = built.load()
    sizes = (C.c_uint64 * 3)()
    lib.prs_rectify_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(built.RectifyMap), C.sizeof(built.RectifyParams), C.sizeof(built.RectifyBatch)]
    M = built.RectifyMap
    assert C.sizeof(M) == 96
    want = dict(model=0, reserved=4, src_fx=8, src_fy=12, src_cx=16, src_cy=20, k1=24, k2=28, p1=32, p2=36, k3=40, R=44, dst_fx=80,
                dst_fy=84, dst_cx=88, dst_cy=92)
    assert {n: getattr(M, n).offset for n, _ in M._fields_} == want
    assert C.sizeof(built.RectifyParams) == 16
    assert [n for n, _ in built.RectifyParams._fields_] == ["pixel_type", "interpolation", "border", "reserved"]
    assert [n for n, _ in built.RectifyBatch._fields_] == ["batch", "src_rows", "src_cols", "src_pitch", "src", "dst_rows", "dst_cols",
                                                          "dst_pitch", "dst", "n_maps", "maps", "map_of", "n_border", "status"]


def test_version_is_still_104(built):
    assert built.load().prs_version() == 104 == built.ABI_VERSION
    assert "#define PRS_ABI_VERSION 104" in open(os.path.join(ROOT, "include", "proslam_hip.h")).read()


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
