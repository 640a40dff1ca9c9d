"""Known answers for the dense RGB-D cloud's numpy restatement (tests/depth_cloud_ref.py), which the kernels are compared with byte
for byte in tests/test_depth_cloud_gpu.py.  No GPU needed."""
import numpy as np
import pytest

import depth_cloud_ref as ref
import ref_pins as rp

F = np.float32
K = dict(fx=525.0, fy=-519.5, cx=18.3, cy=14.7)
IDENTITY = np.eye(4, dtype=F).reshape(1, 16)


def _seq(depth, pose=IDENTITY, **kw):
    depth = np.asarray(depth)
    return dict(depth=depth, n_images=depth.shape[0], pose=np.asarray(pose, F).reshape(-1, 16), **kw)


def _run(seq, p, out_stride=None, **kw):
    frames, rows, cols = seq["depth"].shape
    out = ref.depth_cloud(seq, p, frames * rows * cols if out_stride is None else out_stride, **kw)
    return out, out["xyz"][:out["n_out"]]


def test_constant_depth_is_a_plane():
    d, rows, cols = 2.375, 29, 37
    out, xyz = _run(_seq(np.full((1, rows, cols), d, F)), ref.params(K))
    assert (out["status"], out["n_out"], out["n_total"], out["n_skipped"]) == (ref.PRS_OK, rows * cols, rows * cols, 0)
    assert xyz.dtype == F and (xyz[:, 2] == F(d)).all() and (xyz[:, 3] == 0).all()
    v, u = np.divmod(out["pixel"].astype(np.int64), cols)
    assert out["pixel"].tolist() == list(range(rows * cols)) and (out["frame"] == 0).all()
    cx, cy, fx, fy = (np.float64(F(K[k])) for k in ("cx", "cy", "fx", "fy"))
    x64, y64 = (u - cx) / fx * d, (v - cy) / fy * d
    ulp = np.spacing(F(np.abs(xyz[:, :3]).max()))
    assert np.abs(xyz[:, 0] - x64).max() <= ulp and np.abs(xyz[:, 1] - y64).max() <= ulp


def test_rows_reproject_onto_their_pixels():
    rng = np.random.default_rng(1)
    depth = rng.uniform(0.3, 6.0, (2, 31, 45)).astype(F)
    p = ref.params(K, step=3)
    out, xyz = _run(_seq(depth, np.concatenate([IDENTITY, IDENTITY])), p)
    u = np.rint(xyz[:, 0].astype(np.float64) / xyz[:, 2] * np.float64(p["fx"]) + np.float64(p["cx"])).astype(int)
    v = np.rint(xyz[:, 1].astype(np.float64) / xyz[:, 2] * np.float64(p["fy"]) + np.float64(p["cy"])).astype(int)
    n = out["n_out"]
    assert n == 2 * 11 * 15 and (v * 45 + u == out["pixel"][:n]).all() and (u % 3 == 0).all() and (v % 3 == 0).all()
    assert out["frame"][:n].tolist() == [0] * 165 + [1] * 165


@pytest.fixture(scope="module")
def oracle_backend():
    from test_ref_pins import OracleBackend
    return OracleBackend()


@pytest.mark.parametrize("k", [0, 50])
def test_icl_rows_at_keypoints_are_the_depth_mergers_points(oracle_backend, k):
    """the committed ICL frames: with step 8 the rows whose pixel is a FAST keypoint of the reference's own fixture equal that
    fixture's points -- the depth merger's expression -- bit for bit, and with the frame's pose they equal a float64 evaluation"""
    m = rp.icl_measurements(oracle_backend, k)
    depth = rp.icl_depth_m(k)
    p = ref.params(rp.ICL_K, range_min=0.0, range_max=100.0, step=8)
    out, xyz = _run(_seq(depth[None]), p)
    assert out["status"] == ref.PRS_OK and out["n_skipped"] == 0 and 0 < out["n_out"] <= 60 * 80
    row_of = {int(px): j for j, px in enumerate(out["pixel"][:out["n_out"]])}
    uv = np.rint(m["uv"]).astype(int)
    assert (uv == m["uv"]).all()  # FAST corners are whole pixels
    hits = [(i, row_of[v * 640 + u]) for i, (u, v) in enumerate(uv) if u % 8 == 0 and v % 8 == 0]
    assert len(hits) >= 3
    for i, j in hits:
        assert xyz[j, :3].tobytes() == m["xyz"][i].tobytes(), (i, j)
    # in the world of frame 0: against float64
    T = rp.icl_relative(k)
    out_w, xyz_w = _run(_seq(depth[None], T.astype(F).reshape(1, 16)), p)
    assert out_w["pixel"].tobytes() == out["pixel"].tobytes()
    T32 = T.astype(F).astype(np.float64)
    want = xyz[:, :3].astype(np.float64) @ T32[:3, :3].T + T32[:3, 3]
    # three products and three sums a coordinate, each rounded once: four float32 roundings of terms below the sum of magnitudes
    bound = 4 * np.finfo(F).eps * (np.abs(xyz[:, :3].astype(np.float64)) @ np.abs(T32[:3, :3]).T + np.abs(T32[:3, 3]))
    assert (np.abs(xyz_w[:, :3] - want) <= bound).all()


def test_se3_order_is_that_of_the_other_stages():
    rng = np.random.default_rng(2)
    A, B = rng.normal(size=(4, 4)).astype(F), rng.normal(size=(4, 4)).astype(F)
    T = ref.se3_mul(A, B)
    assert T[0, 1] == F(F(F(A[0, 0] * B[0, 1]) + F(A[0, 1] * B[1, 1])) + F(A[0, 2] * B[2, 1]))
    assert T[2, 3] == F(F(F(F(A[2, 0] * B[0, 3]) + F(A[2, 1] * B[1, 3])) + F(A[2, 2] * B[2, 3])) + A[2, 3])
    assert T[3].tolist() == [0, 0, 0, 1]
    pt = rng.normal(size=(5, 3)).astype(F)
    w = ref.se3_apply(T, pt)
    assert w[3, 1] == F(F(F(F(T[1, 0] * pt[3, 0]) + F(T[1, 1] * pt[3, 1])) + F(T[1, 2] * pt[3, 2])) + T[1, 3])
    assert np.allclose(w, pt.astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3], atol=1e-5)


def test_depth_test_and_range_edges():
    lo, hi = F(0.5), F(2.0)
    values = [0.0, -0.0, np.nan, -1.0, np.inf, np.nextafter(lo, F(0)), lo, np.nextafter(lo, F(1)), np.nextafter(hi, F(0)), hi,
              np.nextafter(hi, F(3)), 1.0]
    depth = np.array(values, F).reshape(1, 3, 4)
    out, xyz = _run(_seq(depth), ref.params(K, range_min=lo, range_max=hi))
    assert out["pixel"][:out["n_out"]].tolist() == [6, 7, 8, 9, 11] and out["n_total"] == 5
    assert xyz[:, 2].tobytes() == np.array([values[i] for i in (6, 7, 8, 9, 11)], F).tobytes()
    # the range is tested on the scaled depth: 16-bit millimetres against metres
    mm = np.array([[0, 499, 500, 501], [1999, 2000, 2001, 65535]], np.uint16).reshape(1, 2, 4)
    p = ref.params(K, range_min=lo, range_max=hi, scale=1e-3)
    out, xyz = _run(_seq(mm), p)
    d = F(1e-3) * mm.reshape(-1).astype(F)
    keep = (d >= lo) & (d <= hi)
    assert out["pixel"][:out["n_out"]].tolist() == np.nonzero(keep)[0].tolist() and xyz[:, 2].tobytes() == d[keep].tobytes()
    assert 2 <= keep.sum() <= 5


def test_order_base_truncation_and_count_only():
    rng = np.random.default_rng(3)
    depth = rng.uniform(0.2, 3.0, (3, 5, 7)).astype(F)
    depth[rng.random(depth.shape) < 0.3] = 0
    pose = np.stack([np.eye(4, dtype=F)] * 3)
    pose[:, 0, 3] = [0, 10, 20]
    gray = rng.integers(0, 256, depth.shape, dtype=np.uint8)
    seq = _seq(depth, pose, gray=gray)
    p = ref.params(K)
    full, xyz = _run(seq, p)
    n = full["n_out"]
    kept = [int((depth[f] > 0).sum()) for f in range(3)]
    assert n == sum(kept) == full["n_total"] and full["frame"][:n].tolist() == sum(([f] * kept[f] for f in range(3)), [])
    key = full["frame"][:n].astype(np.int64) * 35 + full["pixel"][:n]
    assert (np.diff(key) > 0).all()  # image, then raster
    v, u = np.divmod(full["pixel"][:n], 7)
    assert xyz[:, 3].tobytes() == (gray[full["frame"][:n], v, u].astype(F) * (F(1) / F(255))).tobytes()
    # n_base: the rows go behind it, what lies in front and behind n_out stays
    before = dict(xyz=np.full((n + 9, 4), 7, F), frame=np.full(n + 9, -3, np.int32), pixel=np.full(n + 9, -5, np.int32))
    based = ref.depth_cloud(dict(seq, n_base=4), p, n + 9, before=before)
    assert (based["n_out"], based["n_total"], based["status"]) == (n + 4, n + 4, ref.PRS_OK)
    assert based["xyz"][4:n + 4].tobytes() == xyz.tobytes() and (based["xyz"][:4] == 7).all() and (based["xyz"][n + 4:] == 7).all()
    assert (based["frame"][:4] == -3).all() and (based["pixel"][n + 4:] == -5).all()
    # truncation keeps the first rows
    for cap, status in ((n, ref.PRS_OK), (n - 1, ref.PRS_ERR_CAPACITY), (1, ref.PRS_ERR_CAPACITY)):
        cut = ref.depth_cloud(seq, p, cap)
        assert (cut["status"], cut["n_out"], cut["n_total"]) == (status, cap, n) and cut["xyz"].tobytes() == xyz[:cap].tobytes()
    counted = ref.depth_cloud(dict(seq, n_base=2), p, 5, before=dict(xyz=np.full((5, 4), 7, F)), count_only=True)
    assert (counted["status"], counted["n_out"], counted["n_total"]) == (ref.PRS_OK, 2, n + 2) and (counted["xyz"] == 7).all()


def test_skipped_frames_and_refused_sequences():
    depth = np.ones((4, 2, 3), F)
    pose = np.stack([np.eye(4, dtype=F)] * 5).reshape(5, 16)
    pose[:, 3] = np.arange(5)  # x of the translation names the pose
    pose[2, 6] = np.nan
    pose[4, 13] = np.nan  # the bottom row is not looked at
    p = ref.params(dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0))
    out, xyz = _run(_seq(depth, pose, frame_index=[4, 2, 5, 0]), p)
    assert (out["n_skipped"], out["n_out"], out["status"]) == (2, 12, ref.PRS_OK)  # a NaN pose and an index out of range
    assert out["frame"][:12].tolist() == [0] * 6 + [3] * 6 and xyz[::6, 0].tolist() == [4.0, 0.0]
    out, _ = _run(_seq(depth, pose, frame_index=[-1, 1, 1, 3]), p)
    assert (out["n_skipped"], out["n_out"]) == (1, 18)
    short = dict(_seq(depth, pose), n_images=2)
    assert _run(short, p)[0]["n_out"] == 12
    for bad in (dict(n_images=-1), dict(n_images=5), dict(n_base=-1), dict(n_base=25)):
        seq = dict(_seq(depth, pose), **bad)
        out = ref.depth_cloud(seq, p, 24, before=dict(xyz=np.full((24, 4), 7, F)))
        assert (out["status"], out["n_total"], out["n_skipped"]) == (ref.PRS_ERR_RANGE, 0, 0) and (out["xyz"] == 7).all()
        assert out["n_out"] == min(max(bad.get("n_base", 0), 0), 24)


def test_sensor_in_robot_is_applied_on_the_right():
    rng = np.random.default_rng(4)
    depth = rng.uniform(0.5, 2.0, (1, 4, 4)).astype(F)
    S = np.eye(4, dtype=F)
    S[:3, :3] = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]
    S[:3, 3] = [0.1, 0.2, 0.3]
    R = np.eye(4, dtype=F)
    R[:3, 3] = [5, 6, 7]
    _, cam = _run(_seq(depth), ref.params(K))
    _, world = _run(_seq(depth, R.reshape(1, 16)), ref.params(K, sensor_in_robot=S))
    want = (R.astype(np.float64) @ S.astype(np.float64) @ np.concatenate([cam[:, :3], np.ones((16, 1))], axis=1).T).T[:, :3]
    assert np.allclose(world[:, :3], want, atol=1e-5)
