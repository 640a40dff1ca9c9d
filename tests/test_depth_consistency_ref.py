"""The depth consistency filter's numpy restatement (tests/depth_consistency_ref.py) alone, on hand-made cases with exactly
representable numbers and on a synthetic scene with planted outliers.  No GPU needed.  tests/test_depth_consistency_gpu.py runs the
same cases (CASES, scene) on the device."""
import numpy as np
import pytest

import depth_cloud_ref as cloud
import depth_consistency_ref as ref

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
# a camera whose arithmetic is exact on small images: with a depth of 4 the point of pixel (v, u) is (u - 1, v - 1, 4)
CAMERA = dict(fx=4.0, fy=4.0, cx=1.0, cy=1.0)
EYE = np.eye(4, dtype=F).reshape(16)


def at(x, y=0.0, z=0.0):
    T = np.eye(4, dtype=F)
    T[:3, 3] = (x, y, z)
    return T.reshape(16)


def half_turn_about_y():
    T = np.eye(4, dtype=F)
    T[0, 0] = T[2, 2] = F(-1)
    return T.reshape(16)


def run(depth, pose, **kw):
    seq = dict(depth=np.asarray(depth), pose=np.asarray(pose, F), n_images=kw.pop("n_images", None), frame_index=kw.pop("frame_index", None))
    kw.setdefault("window", 1)
    return ref.depth_consistency(seq, ref.params(CAMERA, **kw))


# ---- support, violation, occlusion at the tolerance ----------------------------------------------------------------------------------
def tolerance_case():
    """two frames with the same pose: pixel (v, u) projects onto itself with q2 = 4; max_rel_diff = 0.25 makes tol = 1 exactly"""
    own = np.full((1, 4), 4, F)
    other = np.array([[5, 3, np.nextafter(F(5), INF), np.nextafter(F(3), F(0))]], F)
    return np.stack([own, other]), np.stack([EYE, EYE])


def test_support_violation_and_occlusion_at_the_tolerance():
    depth, pose = tolerance_case()
    r = run(depth, pose, max_rel_diff=0.25, min_support=1, max_violation=0)["results"][0]
    assert r["support"].tolist() == [[1, 1, 0, 0]]      # d_g = 5 and d_g = 3: e = +-1 = +-tol
    assert r["violation"].tolist() == [[0, 0, 1, 0]]    # one ulp above 5: the neighbour sees past the point; one below 3: occluded
    assert r["out"].tolist() == [[4, 4, 0, 0]] and (r["n_kept"], r["n_removed"]) == (2, 2)
    r = run(depth, pose, max_rel_diff=0.25, min_support=0, max_violation=0)["results"][0]
    assert r["out"].tolist() == [[4, 4, 0, 4]]          # occlusion is no vote at all


# ---- the rounding of the projection ---------------------------------------------------------------------------------------------------
def border_case():
    """three frames half a pixel's worth apart along x (depth 4, fx 4: 0.5 m is half a pixel): seen from frame 1, frame 0 (at +0.5)
    sees pixel u at u - 0.5, which rounds to column u -- for u = 0 the projection lies exactly on x + 0.5 == 0 --, and frame 2 (at
    -0.5) sees it at u + 0.5, column u + 1 -- for the last column exactly on cols"""
    return np.full((3, 3, 5), 4, F), np.stack([at(0.5), EYE, at(-0.5)])


def test_projection_on_the_left_border_is_inside_and_on_cols_is_outside():
    depth, pose = border_case()
    r = run(depth, pose, min_support=2)["results"]
    assert (r[1]["support"] == np.array([2, 2, 2, 2, 1], np.uint8)).all()
    assert (r[1]["out"] == np.array([4, 4, 4, 4, 0], F)).all()
    # and the neighbours mark which pixel was hit: with frame 0 empty but for column 0, only u = 0 of frame 1 finds support there
    depth[0, :, 1:] = 0
    r = run(depth, pose, min_support=2)["results"]
    assert (r[1]["support"] == np.array([2, 1, 1, 1, 0], np.uint8)).all()
    # rows likewise
    depth, pose = np.full((3, 5, 2), 4, F), np.stack([at(0, 0.5), EYE, at(0, -0.5)])
    r = run(depth, pose, min_support=2)["results"]
    assert (r[1]["support"] == np.array([2, 2, 2, 2, 1], np.uint8)[:, None]).all()


def test_a_neighbour_that_looks_the_other_way_does_not_vote():
    depth = np.full((2, 3, 3), 4, F)
    r = run(depth, np.stack([EYE, half_turn_about_y()]), min_support=0, max_violation=0)["results"]
    for f in range(2):
        assert not r[f]["support"].any() and not r[f]["violation"].any() and (r[f]["out"] == 4).all()
    assert (ref.relative(EYE.reshape(4, 4), half_turn_about_y().reshape(4, 4))[2, 2]) == -1


# ---- values that are no depth ---------------------------------------------------------------------------------------------------------
def odd_values_case():
    """frame 0 holds the odd values as its own pixels, frame 1 as the neighbour's, the other frame being all 4; same pose"""
    odd = np.array([[NAN, INF, -INF, F(-0.0), F(-4), F(0), F(4), F(11)]], F)
    four = np.full((1, 8), 4, F)
    return np.stack([np.stack([odd, four]), np.stack([four, odd])]), np.stack([EYE, EYE])


def test_nan_inf_negative_zero_and_negative_values():
    (own_odd, neighbour_odd), pose = odd_values_case()
    for depth in (own_odd, neighbour_odd):
        r = run(depth, pose, min_support=1)["results"]
        for f in range(2):
            # only 4 against 4 is a vote: NaN, +-inf, -0, a negative value, 0 and 11 (beyond range_max = 10) are invalid on both sides
            assert r[f]["support"].tolist() == [[0, 0, 0, 0, 0, 0, 1, 0]] and not r[f]["violation"].any()
            assert r[f]["out"].tobytes() == np.array([[0, 0, 0, 0, 0, 0, 4, 0]], F).tobytes()  # -0 comes out as +0
        odd = 0 if depth is own_odd else 1
        assert (r[odd]["n_kept"], r[odd]["n_removed"]) == (1, 0) and (r[1 - odd]["n_kept"], r[1 - odd]["n_removed"]) == (1, 7)


def nan_projection_case():
    """two finite, so usable, poses whose translations differ by more than float32 holds: M's last column of frame 0 is (inf, 0, inf),
    so q2 = inf > 0 and q0 / q2 is NaN, which no comparison admits; seen from frame 1 q2 = -inf"""
    return np.full((2, 2, 2), 4, F), np.stack([at(3e38, 0, 3e38), at(-3e38, 0, -3e38)])


def test_a_projection_that_is_nan_gives_no_vote():
    depth, pose = nan_projection_case()
    M = ref.relative(pose[0].reshape(4, 4), pose[1].reshape(4, 4))
    assert M[0, 3] == INF and M[2, 3] == INF
    r = run(depth, pose, min_support=0, max_violation=0)["results"]
    for f in range(2):
        assert not r[f]["support"].any() and not r[f]["violation"].any() and (r[f]["out"] == 4).all()


# ---- unusable frames ------------------------------------------------------------------------------------------------------------------
def unusable_case():
    """four frames with the same pose but frame 1, whose pose holds a NaN, and frame 3, whose frame_index points outside"""
    depth = np.full((4, 2, 3), 4, F)
    depth[1, 0, 0] = 0
    pose = np.stack([EYE, EYE, EYE, EYE])
    pose[1, 7] = NAN
    return depth, pose, np.array([0, 1, 2, 4], np.int32)


def test_an_unusable_frame_and_an_unusable_neighbour():
    depth, pose, frame_index = unusable_case()
    out = run(depth, pose, frame_index=frame_index, min_support=1, window=1)
    r = out["results"]
    assert out["status"] == ref.PRS_OK and out["n_skipped"] == 2
    for f in (1, 3):
        assert not r[f]["out"].any() and not r[f]["support"].any() and not r[f]["violation"].any() and r[f]["n_kept"] == 0
    assert (r[1]["n_removed"], r[3]["n_removed"]) == (5, 6)  # the valid pixels of the frame
    # frames 0 and 2 have no usable neighbour at window 1, and each other at window 2
    for f in (0, 2):
        assert not r[f]["support"].any() and not r[f]["out"].any() and r[f]["n_removed"] == 6
    r = run(depth, pose, frame_index=frame_index, min_support=1, window=2)["results"]
    for f in (0, 2):
        assert (r[f]["support"] == 1).all() and (r[f]["out"] == 4).all() and r[f]["n_kept"] == 6
    # a bottom row of the pose that is not finite does not matter: the test reads the top three rows
    pose[0, 12:] = NAN
    assert run(depth, pose, frame_index=frame_index)["n_skipped"] == 2


def test_n_images():
    depth, pose = np.full((3, 2, 2), 4, F), np.stack([EYE] * 3)
    out = run(depth, pose, n_images=2, min_support=1)
    assert out["results"][2] is None and (out["results"][1]["support"] == 1).all()  # frame 2 is no neighbour of frame 1
    out = run(depth, pose, n_images=0)
    assert out["status"] == ref.PRS_OK and out["results"] == [None] * 3
    for bad in (-1, 4):
        out = run(depth, pose, n_images=bad)
        assert out["status"] == ref.PRS_ERR_RANGE and out["n_skipped"] == 0 and out["results"] == [None] * 3


def test_stride_and_window_choose_the_slots():
    p = ref.params(CAMERA, window=2, stride=3)
    assert sorted(ref.slots_of(5, p)) == [-1, 2, 8, 11]
    assert sorted(ref.slots_of(0, ref.params(CAMERA, window=8))) == list(range(-8, 0)) + list(range(1, 9))


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_without_a_decision_out_is_the_input_where_valid(dtype):
    rng = np.random.default_rng(3)
    seq, _ = ref.scene()
    depth = seq["depth"].copy()
    depth[rng.random(depth.shape) < 0.2] = 0
    depth[rng.random(depth.shape) < 0.05] = 50
    scale = 1.0
    if dtype == np.uint16:
        depth, scale = np.round(depth * 1000).astype(np.uint16), 1e-3
    else:
        depth[0, 0, :4] = (NAN, INF, F(-0.0), F(-1))
    p = ref.params(ref.SCENE_CAMERA, min_support=0, max_violation=16, scale=scale)
    out = ref.depth_consistency(dict(depth=depth, pose=seq["pose"]), p)
    for f, r in enumerate(out["results"]):
        ok, _ = ref.valid(depth[f], p)
        assert 0 < ok.sum() < ok.size
        assert r["out"].dtype == dtype and r["out"][ok].tobytes() == depth[f][ok].tobytes() and not r["out"][~ok].view(np.uint8).any()
        assert (r["n_kept"], r["n_removed"]) == (ok.sum(), 0)


# ---- the relative transform -----------------------------------------------------------------------------------------------------------
def far_poses():
    """two camera poses a kilometre from the origin, yawed by 0.3, 0.2 m apart: the differences 0.125 and 0.15612495 of the
    translations are exact in float32 (z is small, x has its ulp of 2^-14 at 600), their norm 0.2 to 1e-8"""
    a = ref.yaw_pose(0.3, (600.0, 800.0, 0.0))
    b = ref.yaw_pose(0.3, (600.125, 800.0, 0.15612495))
    return a.reshape(4, 4), b.reshape(4, 4)


def test_the_relative_transform_keeps_a_small_baseline_far_from_the_origin():
    Cg, Cf = far_poses()
    assert abs(np.linalg.norm(Cg[:3, 3].astype(np.float64)) - 1000.0) < 1e-3
    M = ref.relative(Cf, Cg)
    assert M.dtype == F and abs(np.linalg.norm(M[:, 3].astype(np.float64)) - 0.2) < 1e-6
    # the same in float32 throughout -- the inverse of C_g, then the product, as the other stages compose poses -- is not
    Gi = np.eye(4, dtype=F)
    Gi[:3, :3] = Cg[:3, :3].T
    for i in range(3):
        Gi[i, 3] = -F(F(F(Gi[i, 0] * Cg[0, 3]) + F(Gi[i, 1] * Cg[1, 3])) + F(Gi[i, 2] * Cg[2, 3]))
    M32 = cloud.se3_mul(Gi, Cf)
    assert abs(np.linalg.norm(M32[:3, 3].astype(np.float64)) - 0.2) > 1e-6
    # and the rotation part is the identity to float32 rounding: both have the same yaw
    assert np.abs(M[:, :3] - np.eye(3, dtype=F)).max() < 1e-6


def test_relative_of_a_pose_with_itself_is_the_identity():
    Cg, _ = far_poses()
    M = ref.relative(Cg, Cg)
    assert np.abs(M[:, :3] - np.eye(3)).max() < 1e-7 and not M[:, 3].any()


# ---- the synthetic scene --------------------------------------------------------------------------------------------------------------
def test_scene_depth_by_ray_casting():
    d = ref.scene_depth(ref.scene_poses()[2])  # camera 2: at (0, 0.02, 0.1), not yawed
    assert d.shape == (48, 64) and set(np.round(d.astype(np.float64), 5).ravel()) == {2.9, 4.9}
    assert d[24, 32] == F(2.9) and d[0, 0] == F(4.9)
    # the rectangle spans |x| <= 0.6 at z = 3: columns 31.5 +- 0.6 / 2.9 * 60
    assert (d[24] == F(2.9)).sum() == 24


def test_quality_on_the_synthetic_scene():
    """planted outliers (5 % of the pixels, depth times a factor in [0.5, 0.8] or [1.25, 2]) are removed, clean pixels are kept"""
    seq, planted = ref.scene()
    assert 0.03 < planted.mean() < 0.07
    out = ref.depth_consistency(seq, ref.params(ref.SCENE_CAMERA, window=2, stride=1, max_rel_diff=0.02, min_support=2, max_violation=1))
    kept = np.stack([r["out"] > 0 for r in out["results"]])
    planted_surviving = kept[planted].mean()
    clean_surviving = kept[2][~planted[2]].mean()
    print("planted pixels surviving %.4f, clean pixels of frame 2 surviving %.4f" % (planted_surviving, clean_surviving))
    assert planted_surviving <= 0.02
    assert clean_surviving >= 0.85
