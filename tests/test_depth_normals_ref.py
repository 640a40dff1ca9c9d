"""The depth normals' rule itself (tests/depth_normals_ref.py, the numpy restatement of include/proslam_hip_normals.h): exact results
on fronto-parallel planes, the depth-edge gate, the properties and the accuracy of the float32 rule on a tilted plane and a sphere,
the values that are not depths, smoothing, and the cloud rows.  No GPU needed."""
import numpy as np
import pytest

import depth_normals_cases as cases
import depth_normals_ref as ref

F = np.float32
K = cases.K
SETTINGS = ((1, 0), (2, 1), (8, 3))


def normals(image, camera=K, **kw):
    return ref.normals_image(image, ref.params(camera, **kw))


def test_constant_depth_gives_the_optical_axis_exactly():
    for r in (1, 2, 3):
        for s in (0, 1):
            out = normals(np.full((11, 13), 1.5, F), radius=r, smooth=s)
            assert np.array_equal(out[..., :3], np.broadcast_to(F([0, 0, -1]), (11, 13, 3))), (r, s)
            w = out[..., 3]
            assert (w[r:-r, r:-r] == 4).all()
            assert (w[:r, r:-r] == 3).all() and (w[-r:, r:-r] == 3).all() and (w[r:-r, :r] == 3).all() and (w[r:-r, -r:] == 3).all()
            assert (w[:r, :r] == 2).all() and (w[:r, -r:] == 2).all() and (w[-r:, :r] == 2).all() and (w[-r:, -r:] == 2).all()
    u16 = normals(np.full((5, 5), 1500, np.uint16), radius=1, smooth=0, scale=1e-3)
    assert np.array_equal(u16[2, 2], F([0, 0, -1, 4]))


@pytest.mark.parametrize("shape", [(1, 9), (9, 1), (1, 1)])
def test_an_image_of_one_row_or_column_has_no_normal(shape):
    for r, s in SETTINGS:
        assert not normals(np.full(shape, 2.0, F), radius=r, smooth=s).any()


def test_an_image_narrower_than_the_radius():
    out = normals(np.full((20, 3), 2.0, F), radius=8, smooth=0)  # no left or right neighbour anywhere
    assert not out.any()
    out = normals(np.full((20, 9), 2.0, F), radius=8, smooth=0)  # only the first and the last column have one
    assert (out[:, (0, 8), 3] > 0).all() and not out[:, 1:8].any()


def test_a_depth_step_is_not_differenced_across():
    """near | far with a step of 50 %: beside the step the differences are one-sided and the normal stays exact; with the gate
    widened past the step the central difference spans it and the normal tilts"""
    d = cases.step_image(9, 12, 2.0, 3.0, 6)
    for r in (1, 2):
        out = normals(d, radius=r, smooth=0, max_rel_diff=0.05)
        assert np.array_equal(out[..., :3], np.broadcast_to(F([0, 0, -1]), (9, 12, 3)))
        assert (out[r:-r, 6 - r:6 + r, 3] == 3).all() and (out[r:-r, r:6 - r, 3] == 4).all() and (out[r:-r, 6 + r:-r, 3] == 4).all()
        wide = normals(d, radius=r, smooth=0, max_rel_diff=0.6)
        assert (wide[r:-r, r:-r, 3] == 4).all()
        beside = wide[r:-r, 6 - r:6 + r, :3]
        assert (np.abs(beside[..., 0]) > 0.5).all() and (beside[..., 2] > -0.9).all()
    # the gate is relative to the centre's depth: 2 -> 2.9 is 45 % seen from the near side and 31 % seen from the far side
    one_way = normals(cases.step_image(5, 8, 2.0, 2.9, 4), radius=1, smooth=0, max_rel_diff=0.4)
    assert one_way[2, 3, 3] == 3 and one_way[2, 4, 3] == 4


def scene(kind, seed):
    """(float32 depth, camera, the mask of the pixels the test looks at, the true normals facing the camera [rows, cols, 3])"""
    rng = np.random.default_rng([11, seed])
    if kind == "plane":
        camera = K if seed % 2 else cases.K_WIDE
        tilt = rng.uniform(-0.35, 0.35, 2)
        d, n = cases.plane_depth(48, 64, camera, (tilt[0], tilt[1], 1.0), rng.uniform(1.5, 3.0))
        return d, camera, np.ones(d.shape, bool), np.broadcast_to(n, d.shape + (3,))
    d, X, hit = cases.sphere_depth(48, 64, cases.K_WIDE, rng.uniform(2.5, 3.5), rng.uniform(0.8, 1.2))
    return d, cases.K_WIDE, hit, X


# the largest angle between the float32 rule and the same rule in float64 over both scenes at seed 0, in radians, per (radius,
# smooth); the test allows four times that for the other seeds
MEASURED_ANGLE = {(1, 0): 9.97e-7, (2, 1): 2.90e-7, (8, 3): 2.01e-7}


@pytest.mark.parametrize("kind", ["plane", "sphere"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_properties_and_accuracy_on_a_tilted_plane_and_a_sphere(kind, seed):
    d, camera, mask, truth = scene(kind, seed)
    kx, ky = cases.rays(d.shape[0], d.shape[1], camera)
    points = np.stack([kx * d, ky * d, d.astype(np.float64)], axis=-1)
    for r, s in SETTINGS:
        out = ref.normals_image(d, ref.params(camera, r, s, max_rel_diff=0.2))
        exact = ref.normals_image(d, ref.params(camera, r, s, max_rel_diff=0.2, dtype=np.float64))
        assert out.dtype == F and exact.dtype == np.float64
        has = out[..., 3] > 0
        assert np.array_equal(has, exact[..., 3] > 0) and np.array_equal(out[..., 3], exact[..., 3])
        assert has[mask].mean() > 0.8
        n = out[has][:, :3].astype(np.float64)
        assert ((n * points[has]).sum(-1) <= 0).all()                     # it faces the camera
        assert np.abs((n * n).sum(-1) - 1.0).max() <= 1e-6                # three rounded divisions, one sqrtf, a three-term sum
        angle = ref.angle_between(n, exact[has][:, :3]).max()
        print("%s seed %d radius %d smooth %d: %.3g rad against float64" % (kind, seed, r, s, angle))
        assert angle <= 4 * MEASURED_ANGLE[(r, s)], (r, s, angle)
        # and the rule finds the surface: away from the image border, the rim and (for the sphere) over a chord of 2 r pixels
        inner = has & mask
        inner[:r + s] = inner[-(r + s):] = False
        inner[:, :r + s] = inner[:, -(r + s):] = False
        for dv, du in ((-r - s, 0), (r + s, 0), (0, -r - s), (0, r + s)):
            inner &= ref.shifted(mask & has, dv, du, False)
        assert inner.sum() > 20
        assert ref.angle_between(out[inner][:, :3], truth[inner]).max() <= (1e-4 if kind == "plane" else 0.2)


def test_values_that_are_not_depths():
    d, odd = cases.odd_values_image(np.random.default_rng(5))
    with np.errstate(all="ignore"):
        out = normals(d, radius=1, smooth=0)
    assert not out[odd].any()                        # no normal of their own
    has = out[..., 3] > 0
    assert has.any() and np.array_equal(out[has][:, :3], np.broadcast_to(F([0, 0, -1]), (int(has.sum()), 3)))
    # w counts the neighbours that are valid: the same image with the odd values as plain holes gives the same result
    holes = np.where(odd, F(0), d)
    assert normals(holes, radius=1, smooth=0).tobytes() == out.tobytes()
    ok = ~odd
    count = sum(ref.shifted(ok, dv, du, False).astype(int) for dv, du in ((0, -1), (0, 1), (-1, 0), (1, 0)))
    assert np.array_equal(out[..., 3][has], count[has].astype(F))
    # the range is tested on the product: 16-bit millimetres outside [0.5, 2] m
    u = np.full((3, 8), 1000, np.uint16)
    u[1] = [0, 1, 499, 500, 2000, 2001, 65535, 1000]
    p = ref.params(K, 1, 0, scale=1e-3, range_min=0.5, range_max=2.0, max_rel_diff=10.0)
    assert (~np.isnan(ref.metres(u, p)[1])).tolist() == [False, False, False, True, True, False, False, True]
    # the row above has them as its only vertical neighbours: no normal over an invalid one, w = 3 (2 in the corner) over a valid one
    assert ref.normals_image(u, p)[0, :, 3].tolist() == [0, 0, 0, 3, 3, 0, 0, 2]


def test_products_that_are_denormal():
    """tangents so short that m_i * m_i underflows: len2 is a denormal or 0, and the rule says which"""
    cam = dict(fx=1e18, fy=1e18, cx=0.0, cy=0.0)
    d = np.full((3, 3), 1.0, F)
    out = normals(d, cam, radius=1, smooth=0)
    assert not out.any()                                  # m2 = 4e-36 is normal, its square 1.6e-71 is 0: no normal
    cam = dict(fx=3e10, fy=3e10, cx=0.0, cy=0.0)
    out = normals(d, cam, radius=1, smooth=0)             # m2 = 4.4e-21, its square 2e-41 is a denormal
    tiny = np.finfo(F).tiny
    m2 = F(F(2) / F(3e10)) * F(F(2) / F(3e10))
    assert m2 >= tiny and 0 < F(m2 * m2) < tiny
    # a denormal holds few bits, so the length is rounded coarsely: the normal is the axis to 1e-4, not exactly
    assert (out[..., 3] > 0).all() and np.array_equal(out[1, 1, (0, 1, 3)], F([0, 0, 4])) and abs(out[1, 1, 2] + 1) < 1e-4


def test_smoothing():
    rng = np.random.default_rng(6)
    d = cases.random_depth(rng, (20, 30), "f32")
    p0 = ref.params(K, 2, 0)
    metres = ref.metres(d, p0)
    n, w, has = ref.raw_normals(metres, p0)
    raw = ref.normals_image(d, p0)
    assert np.array_equal(raw[..., :3], n.transpose(1, 2, 0)) and np.array_equal(raw[..., 3], w)   # smooth 0 is the raw rule
    assert 0.3 < has.mean() < 0.95
    out = ref.normals_image(d, ref.params(K, 2, 2))
    assert not out[~has].any()                                                                       # no raw normal: none
    kept = out[..., 3] > 0
    assert kept.sum() > 0.9 * has.sum() and np.array_equal(out[..., 3][kept], w[kept])               # w stays the centre's
    assert np.abs((out[kept][:, :3].astype(np.float64) ** 2).sum(-1) - 1).max() <= 1e-6
    # the window's gate: two planes of different tilt that meet in a step; a pixel beside the step keeps its own side's normal
    left, nl = cases.plane_depth(16, 24, cases.K_WIDE, (0.3, 0.0, 1.0), 2.0)
    right, nr = cases.plane_depth(16, 24, cases.K_WIDE, (-0.3, 0.1, 1.0), 3.2)
    both = np.concatenate([left[:, :12], right[:, 12:]], axis=1)
    assert (right[:, 12] > 1.3 * left[:, 11]).all()
    gated = ref.normals_image(both, ref.params(cases.K_WIDE, 1, 3, max_rel_diff=0.1))
    assert ref.angle_between(gated[3:-3, 3:12, :3], nl).max() < 1e-4 and ref.angle_between(gated[3:-3, 12:-3, :3], nr).max() < 1e-4
    open_gate = ref.normals_image(both, ref.params(cases.K_WIDE, 1, 3, max_rel_diff=0.9))
    assert ref.angle_between(open_gate[3:-3, 9:12, :3], nl).min() > 0.05


def rows_case():
    rng = np.random.default_rng(7)
    depth = cases.random_depth(rng, (3, 6, 8), "f32", invalid=0.0)
    pose = np.tile(np.eye(4, dtype=F).reshape(16), (4, 1))
    pose[1].reshape(4, 4)[:3, :3] = F([[0, -1, 0], [1, 0, 0], [0, 0, 1]])
    pose[1].reshape(4, 4)[:3, 3] = F([100, 200, 300])
    seq = dict(depth=depth, n_images=2, pose=pose, frame_index=np.array([1, 0, 2], np.int32))
    frame = np.array([0, 0, 1, 1, 0, 1, 0, 1], np.int32)
    pixel = np.array([9, 10, 9, 47, 20, 21, 22, 23], np.int32)
    return seq, dict(frame=frame, pixel=pixel, n=7, base=None)


def test_rows():
    seq, rows = rows_case()
    p = ref.params(K, 1, 0, max_rel_diff=0.5)
    before = dict(row_normal=np.full((8, 4), 7.0, F))
    out = ref.depth_normals(seq, p, before, rows)
    assert out["status"] == ref.PRS_OK and out["n_bad_rows"] == 0
    normal = out["normal"]
    assert (normal[:2, ..., 3] > 0).any() and not normal[2].any()          # the image behind n_images is not written
    n0 = normal[0].reshape(-1, 4)[9]
    assert n0[3] > 0
    # image 0 has pose 1: a quarter turn about z, and a translation that a direction ignores
    assert np.array_equal(out["row_normal"][0], F([-n0[1], n0[0], n0[2], n0[3]]))
    assert np.array_equal(out["row_normal"][2], normal[1].reshape(-1, 4)[9])  # image 1 has pose 0: the identity
    assert (out["row_normal"][7] == 7.0).all()                              # behind row_n: untouched
    for name, change in (("frame", dict(frame=2)), ("frame", dict(frame=-1)), ("pixel", dict(pixel=48)), ("pixel", dict(pixel=-1))):
        bad = dict(rows, frame=rows["frame"].copy(), pixel=rows["pixel"].copy())
        for k, v in change.items():
            bad[k][3] = v
        got = ref.depth_normals(seq, p, before, bad)
        assert got["n_bad_rows"] == 1 and not got["row_normal"][3].any() and got["row_normal"][4].any(), (name, change)
    for index in (4, -1):  # frame_index out of [0, pose_stride)
        got = ref.depth_normals(dict(seq, frame_index=np.array([1, index, 2], np.int32)), p, before, rows)
        assert got["n_bad_rows"] == 3 and not got["row_normal"][[2, 3, 5]].any()
    nan_pose = seq["pose"].copy()
    nan_pose[0, 7] = np.nan
    got = ref.depth_normals(dict(seq, pose=nan_pose), p, before, rows)
    assert got["n_bad_rows"] == 3 and got["row_normal"][0].any()
    nan_pose = seq["pose"].copy()
    nan_pose[0, 13] = np.nan                                                # the bottom row is not looked at
    assert ref.depth_normals(dict(seq, pose=nan_pose), p, before, rows)["n_bad_rows"] == 0
    # row_base leaves the rows below it as they are
    got = ref.depth_normals(seq, p, before, dict(rows, base=3))
    assert (got["row_normal"][:3] == 7.0).all() and np.array_equal(got["row_normal"][3:7], out["row_normal"][3:7])
    # the refusals write nothing
    for refused in (dict(rows, n=9), dict(rows, n=-1), dict(rows, base=8), dict(rows, base=-1), dict(rows, base=5, n=4)):
        got = ref.depth_normals(seq, p, dict(before, normal=np.full((3, 6, 8, 4), 5.0, F)), refused)
        assert got["status"] == ref.PRS_ERR_RANGE and (got["normal"] == 5.0).all() and (got["row_normal"] == 7.0).all()
    for n_images in (-1, 4):
        assert ref.depth_normals(dict(seq, n_images=n_images), p)["status"] == ref.PRS_ERR_RANGE
