"""The TSDF fusion's restatement (tests/tsdf_ref.py) on cases whose answer is known without it: a fronto-parallel plane, weight
saturation, the chunk property, a skipped frame, the band gate at a depth step, and the sphere scene of the stage's design as a
condition.  No GPU needed."""
import numpy as np

import tsdf_cases as cases
import tsdf_ref as ref

F = np.float32
CAM = dict(fx=40.0, fy=40.0, cx=31.5, cy=23.5)
ROWS, COLS = 48, 64
EYE = np.eye(4, dtype=F).reshape(1, 16)


def plane_case(frames=1, depth=2.0, max_weight=64.0):
    """8 x 6 x 16 voxels of 1/8 m about the optical axis, from z = 1; a plane at `depth` seen from the identity pose.  Every
    number is a small multiple of a power of two: the rule is exact"""
    p = ref.params(CAM, voxel_size=0.125, truncation=0.5, max_weight=max_weight, range_min=0.25, range_max=8.0)
    seq = dict(depth=np.full((frames, ROWS, COLS), depth, F), pose=np.tile(EYE, (frames, 1)))
    origin = np.array([-0.5, -0.375, 1.0, 0.0], F)
    return seq, p, origin, np.zeros((16, 6, 8, 2), F)


def test_plane_from_the_identity_pose_is_linear_in_k_and_crosses_on_the_plane():
    seq, p, origin, empty = plane_case()
    out = ref.integrate(seq, p, origin, empty)
    assert out["status"] == 0 and out["n_skipped"] == 0
    z = 1.0 + (np.arange(16) + 0.5) * 0.125                   # the centres' depth: exact in float32
    want_t = np.minimum((2.0 - z) / 0.5, 1.0)
    seen = (2.0 - z) >= -0.5                                   # behind the band: never updated
    assert seen.sum() == 12 and out["n_updates"].tolist() == [12 * 48]
    for k in range(16):
        assert (out["volume"][k, :, :, 1] == (1.0 if seen[k] else 0.0)).all()
        assert (out["volume"][k, :, :, 0] == (F(want_t[k]) if seen[k] else 0.0)).all()
    s = ref.surface(out["volume"], p, origin, 100)
    assert (s["status"], s["n_total"], s["n_out"]) == (0, 48, 48)  # one crossing a column, between z = 1.9375 and 2.0625
    assert (s["xyz"][:48, 2] == 2.0).all() and (s["xyz"][:48, 3] == 1.0).all()
    assert (s["normal"][:48] == np.array([0, 0, -1, 1], F)).all()  # towards the camera
    i, j = np.meshgrid(np.arange(8), np.arange(6), indexing="xy")
    assert s["cell"][:48].tolist() == (3 * ((7 * 6 + j.reshape(-1)) * 8 + i.reshape(-1)) + 2).tolist()
    assert (s["xyz"][:48, 0] == (-0.5 + (i.reshape(-1) + 0.5) * 0.125)).all()
    assert (s["xyz"][48:] == 0).all()
    # a plane on a voxel centre: tsdf 0 is not negative, the crossing lies between that voxel and the next, at s = 0
    seq["depth"][:] = 2.0625
    on = ref.surface(ref.integrate(seq, p, origin, empty)["volume"], p, origin, 100)
    assert on["n_total"] == 48 and (on["xyz"][:48, 2] == 2.0625).all() and (on["cell"][:48] // 3 // 48 == 8).all()


def test_weight_saturates_at_max_weight():
    seq, p, origin, empty = plane_case(frames=5, max_weight=3.0)
    out = ref.integrate(seq, p, origin, empty)
    once = ref.integrate(dict(seq, n_images=1), p, origin, empty)
    assert out["n_updates"].tolist() == [12 * 48] * 5 and once["n_updates"].tolist() == [12 * 48, 0, 0, 0, 0]
    assert set(np.unique(out["volume"][..., 1])) == {0.0, 3.0}
    assert out["volume"][..., 0].tobytes() == once["volume"][..., 0].tobytes()  # the mean of equal quarters is exact
    # at the cap a new measurement keeps a quarter of the say: (t * 3 + t') / 4
    seq["depth"][4] = 2.25
    moved = ref.integrate(seq, p, origin, empty)["volume"]
    assert moved[7, 0, 0].tolist() == [(0.125 * 3 + 0.625) / 4, 3.0]


def random_case(rng, frames=4, depth_type="f32"):
    p = ref.params(cases.K, voxel_size=0.06, truncation=0.2, max_weight=3.0, scale=1e-3 if depth_type == "u16" else 1.0,
                   sensor_in_robot=cases.random_pose(rng, 0.1))
    pose = np.stack([cases.random_pose(rng, 0.2).reshape(16) for _ in range(frames)])
    for T in pose:  # look roughly down the world's z
        T.reshape(4, 4)[:3, :3] = cases.rot_y(rng.uniform(-0.3, 0.3)).astype(F)
    p["sensor_in_robot"][:3, :3] = np.eye(3, dtype=F)
    seq = dict(depth=cases.wavy_depth(rng, frames, depth_type=depth_type), pose=pose)
    origin = np.array([-0.6, -0.5, 0.6, 7.0], F)
    return seq, p, origin, (20, 17, 21)


def test_two_calls_equal_one_call():
    rng = np.random.default_rng(5)
    seq, p, origin, (nz, ny, nx) = random_case(rng)
    empty = np.zeros((nz, ny, nx, 2), F)
    whole = ref.integrate(seq, p, origin, empty)
    assert min(whole["n_updates"]) > 200 and whole["volume"][..., 1].max() == 3.0
    first = ref.integrate(dict(depth=seq["depth"][:2], pose=seq["pose"][:2]), p, origin, empty)
    second = ref.integrate(dict(depth=seq["depth"][2:], pose=seq["pose"][2:]), p, origin, first["volume"])
    assert second["volume"].tobytes() == whole["volume"].tobytes()
    assert first["n_updates"].tolist() + second["n_updates"].tolist() == whole["n_updates"].tolist()
    # a voxel that no image reaches keeps its bytes, whatever they are
    marked = np.full_like(empty, -7.5)
    out = ref.integrate(seq, p, origin, marked)["volume"]
    untouched = whole["volume"][..., 1] == 0
    assert untouched.any() and (out[untouched] == -7.5).all() and not (out[~untouched] == -7.5).all()


def test_a_nan_pose_is_skipped_and_counted_and_a_bad_n_images_refused():
    rng = np.random.default_rng(6)
    seq, p, origin, (nz, ny, nx) = random_case(rng)
    empty = np.zeros((nz, ny, nx, 2), F)
    seq["pose"][1, 7] = np.nan
    seq["frame_index"] = np.array([0, 1, 2, 9], np.int32)  # the last one has no pose
    out = ref.integrate(seq, p, origin, empty)
    assert out["status"] == 0 and out["n_skipped"] == 2 and out["n_updates"][1] == 0 and out["n_updates"][3] == 0
    without = ref.integrate(dict(depth=seq["depth"][[0, 2]], pose=seq["pose"][[0, 2]]), p, origin, empty)
    assert out["volume"].tobytes() == without["volume"].tobytes()
    seq["pose"][1, 14] = np.inf  # the bottom row is not read
    for bad in (-1, 5):
        before = np.array([9, 9, 9, 9], np.int32)
        refused = ref.integrate(dict(seq, n_images=bad), p, origin, empty + 2, before)
        assert refused["status"] == ref.PRS_ERR_RANGE and refused["n_skipped"] == 0
        assert (refused["volume"] == 2).all() and refused["n_updates"].tolist() == [9] * 4


def test_band_gate_keeps_a_depth_step_from_becoming_a_sheet():
    """the left half of the image sees a wall at 1.5 m, the right half one at 2.5 m: beside the step, voxels behind the near wall
    (tsdf < 0) have truncated free space (tsdf 1) as their x neighbour"""
    seq, p, origin, empty = plane_case()
    seq["depth"][:, :, :COLS // 2] = 1.5
    seq["depth"][:, :, COLS // 2:] = 2.5
    vol = ref.integrate(seq, p, origin, empty)["volume"]
    t, w = vol[..., 0], vol[..., 1]
    jump = (w[:, :, :-1] > 0) & (w[:, :, 1:] > 0) & ((t[:, :, :-1] < 0) != (t[:, :, 1:] < 0))
    assert jump.sum() >= 6 * 3 and (np.maximum(np.abs(t[:, :, :-1]), np.abs(t[:, :, 1:]))[jump] == 1.0).all()
    s = ref.surface(vol, p, origin, 200)
    n = s["n_out"]
    assert s["status"] == 0 and n == s["n_total"] == 48                   # one crossing a column, none along x
    assert (s["cell"][:n] % 3 == 2).all()
    near = s["xyz"][:n, 0] < 0
    assert near.sum() == 24 and (s["xyz"][:n, 2][near] == 1.5).all() and (s["xyz"][:n, 2][~near] == 2.5).all()


def test_min_weight_and_capacity():
    seq, p, origin, empty = plane_case(frames=2)
    vol = ref.integrate(seq, p, origin, empty)["volume"]
    assert ref.surface(vol, dict(p, min_weight=F(2.0)), origin, 100)["n_total"] == 48
    assert ref.surface(vol, dict(p, min_weight=F(2.5)), origin, 100)["n_total"] == 0
    before = dict(xyz=np.full((40, 4), 5, F), normal=np.full((40, 4), 6, F), cell=np.full(40, 7, np.int32))
    full = ref.surface(vol, p, origin, 48)
    short = ref.surface(vol, p, origin, 40, before)
    assert (full["status"], full["n_out"]) == (0, 48) and (short["status"], short["n_out"], short["n_total"]) == (ref.PRS_ERR_CAPACITY, 40, 48)
    assert short["xyz"].tobytes() == full["xyz"][:40].tobytes() and short["cell"].tobytes() == full["cell"][:40].tobytes()
    count = ref.surface(vol, p, origin, 40, before, count_only=True)
    assert (count["status"], count["n_out"], count["n_total"]) == (0, 0, 48) and (count["xyz"] == 5).all() and (count["cell"] == 7).all()


def test_sphere_from_four_views_lies_within_a_voxel():
    """a condition on the rule, not a measurement: every point within one voxel of the sphere, at least 500 of them.  As the scene is
    placed here (the volume centred on the sphere, the cameras 2 m from its centre) the rule gives 898 points and a worst error of
    0.88 voxels, at the silhouettes, where the distance along z overstates the distance to the surface"""
    s = cases.SPHERE
    seq, origin = cases.sphere_scene()
    nx, ny, nz = s["dims"]
    p = ref.params(s["camera"], voxel_size=s["voxel_size"], truncation=s["truncation"])
    out = ref.integrate(seq, p, origin, np.zeros((nz, ny, nx, 2), F))
    assert out["status"] == 0 and out["n_skipped"] == 0 and min(out["n_updates"]) > 1000
    surf = ref.surface(out["volume"], p, origin, 3 * nx * ny * nz)
    n = surf["n_out"]
    points = surf["xyz"][:n, :3].astype(np.float64)
    error = np.abs(np.linalg.norm(points - np.array(s["centre"]), axis=1) - s["radius"])
    print("sphere: %d points, worst error %.3f voxels" % (n, error.max() / s["voxel_size"]))
    assert n >= 500
    assert error.max() <= s["voxel_size"]
    # the normals point out of the sphere, to the free side
    radial = (points - np.array(s["centre"])) / s["radius"]
    has = surf["normal"][:n, 3] > 0
    outward = (surf["normal"][:n, :3] * radial).sum(1)
    print("sphere: least normal . radius %.3f, median %.3f" % (outward.min(), np.median(outward)))
    assert has.all() and (outward > 0).all() and np.median(outward) > 0.95
