"""The TSDF raycast's restatement (tests/tsdf_raycast_ref.py) on cases whose answer is known without it: the sphere scene of the fusion
stage rendered from four poses against the analytic depth and normal, volumes that hold no surface, and the skip, refusal and
untouched-view rules.  No GPU needed."""
import numpy as np
import pytest

import tsdf_cases as cases
import tsdf_raycast_ref as ref
import tsdf_ref

F = np.float32
S = cases.SPHERE


@pytest.fixture(scope="module")
def sphere_volume():
    """the sphere scene fused by the fusion's restatement -> (volume, origin)"""
    seq, origin = cases.sphere_scene()
    nx, ny, nz = S["dims"]
    p = tsdf_ref.params(S["camera"], voxel_size=S["voxel_size"], truncation=S["truncation"])
    return tsdf_ref.integrate(seq, p, origin, np.zeros((nz, ny, nx, 2), F))["volume"], origin


def sphere_views():
    seq, _ = cases.sphere_scene()
    return np.stack([seq["pose"][0], seq["pose"][1], cases.pose_about(S["centre"], 0.25, 2.0), cases.pose_about(S["centre"], -0.2, 1.6)])


def analytic_normal(pose, truth):
    """the sphere's outward normal at the truth's points, in the camera's frame [rows, cols, 3]"""
    T = np.asarray(pose, np.float64).reshape(4, 4)
    cam = S["camera"]
    v, u = np.meshgrid(np.arange(S["rows"]), np.arange(S["cols"]), indexing="ij")
    pc = np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones(u.shape)], axis=-1) * truth[..., None].astype(np.float64)
    centre = T[:3, :3].T @ (np.asarray(S["centre"], np.float64) - T[:3, 3])
    return (pc - centre) / S["radius"]


@pytest.mark.parametrize("step", [0.05, 0.025])
def test_sphere_depth_and_normals_against_the_analytic_sphere(sphere_volume, step):
    """the conditions of the stage's design, per view: coverage >= 0.88, false hits <= 3 %, mean error <= 0.2 voxel, 95th percentile
    <= 0.6 voxel, errors over a voxel <= 1 %, normals on >= 80 % of the hits, every cosine >= 0.8, and the 1st percentile of the
    cosines pooled over the views >= 0.95"""
    volume, origin = sphere_volume
    poses = sphere_views()
    p = ref.params(S["camera"], voxel_size=S["voxel_size"], step=step)
    out = ref.raycast(dict(pose=poses), p, origin, volume, len(poses), S["rows"], S["cols"])
    assert out["status"] == 0 and out["n_skipped"] == 0
    pooled = []
    for r, pose in enumerate(poses):
        truth = cases.sphere_depth(pose, S["camera"], S["rows"], S["cols"], S["centre"], S["radius"])
        d, nrm = out["depth"][r], out["normal"][r]
        there, got = truth > 0, d > 0
        assert out["n_hit"][r] == got.sum()
        both = there & got
        coverage, false_hits = both.sum() / there.sum(), (got & ~there).sum() / there.sum()
        err = np.abs(d[both].astype(np.float64) - truth[both]) / S["voxel_size"]
        has = nrm[..., 3] > 0
        assert not (has & ~got).any() and set(np.unique(nrm[..., 3])) <= {0.0, 1.0}
        cos = (nrm[..., :3].astype(np.float64) * analytic_normal(pose, truth)).sum(-1)[has & both]
        pooled.append(cos)
        print("step %.3f view %d: coverage %.3f, false hits %.3f, error mean %.3f p95 %.3f max %.3f voxels, over a voxel %.4f, normals on "
              "%.3f of the hits, least cosine %.3f" % (step, r, coverage, false_hits, err.mean(), np.percentile(err, 95), err.max(),
                                                        (err > 1).mean(), has.sum() / got.sum(), cos.min()))
        assert coverage >= 0.88
        assert false_hits <= 0.03
        assert err.mean() <= 0.2
        assert np.percentile(err, 95) <= 0.6
        assert (err > 1).mean() <= 0.01
        assert has.sum() / got.sum() >= 0.8
        assert cos.min() >= 0.8
    first = np.percentile(np.concatenate(pooled), 1)
    print("step %.3f: 1st percentile of the cosines %.3f" % (step, first))
    assert first >= 0.95


CAM = dict(fx=30.0, fy=29.0, cx=11.3, cy=9.6)
ROWS, COLS = 20, 24


def plane_volume(dims=(12, 10, 16), vs=0.125, z_plane=2.0, trunc=0.5):
    """(volume, origin): a plane at z_plane seen from the identity pose, every voxel observed once"""
    nx, ny, nz = dims
    z = 1.0 + (np.arange(nz) + 0.5) * vs
    t = np.clip((z_plane - z) / trunc, -1.0, 1.0).astype(F)
    volume = np.zeros((nz, ny, nx, 2), F)
    volume[..., 0], volume[..., 1] = t[:, None, None], 1.0
    return volume, np.array([-nx * vs / 2, -ny * vs / 2, 1.0, 0.0], F)


def test_a_plane_is_rendered_at_its_depth_with_its_normal():
    volume, origin = plane_volume()
    p = ref.params(CAM, voxel_size=0.125, step=0.125)
    out = ref.raycast(dict(pose=np.eye(4, dtype=F).reshape(1, 16)), p, origin, volume, 1, ROWS, COLS)
    d, n = out["depth"][0], out["normal"][0]
    assert (d > 0).sum() == out["n_hit"][0] > 100
    assert np.abs(d[d > 0] - 2.0).max() < 1e-5                 # the tsdf is linear in z: the interpolation is exact up to rounding
    has = n[..., 3] > 0
    assert has.sum() > 50 and np.abs(n[has][:, :3] - np.array([0, 0, -1], F)).max() < 1e-5  # towards the camera
    assert (n[~has] == 0).all() and not (has & (d == 0)).any()


def test_volumes_without_a_surface_give_no_hit():
    _, origin = plane_volume()
    p = ref.params(CAM, voxel_size=0.125, step=0.125)
    seq = dict(pose=np.eye(4, dtype=F).reshape(1, 16))
    empty = ref.raycast(seq, p, origin, np.zeros((16, 10, 12, 2), F), 1, ROWS, COLS)
    assert (empty["depth"] == 0).all() and (empty["normal"] == 0).all() and empty["n_hit"].tolist() == [0]
    volume, origin = plane_volume(dims=(12, 1, 16))            # no cell along y: no sample is valid
    flat = ref.raycast(seq, p, origin, volume, 1, ROWS, COLS)
    assert (flat["depth"] == 0).all() and (flat["normal"] == 0).all() and flat["n_hit"].tolist() == [0] and flat["status"] == 0


def test_skipped_refused_and_untouched_views():
    volume, origin = plane_volume()
    p = ref.params(CAM, voxel_size=0.125, step=0.125)
    eye = np.eye(4, dtype=F).reshape(16)
    bad = eye.copy()
    bad[7] = np.nan
    pose = np.stack([eye, bad, eye])
    full = lambda shape, dtype: np.full(shape, 7, dtype)  # noqa: E731
    before = dict(depth=full((4, ROWS, COLS), F), normal=full((4, ROWS, COLS, 4), F), n_hit=full((4,), np.int32))
    seq = dict(pose=pose, view_index=np.array([2, 1, 5, 0], np.int32), n_views=3)
    out = ref.raycast(seq, p, origin, volume, 4, ROWS, COLS, before)
    assert out["status"] == 0 and out["n_skipped"] == 2        # the NaN pose and the index out of range
    assert out["n_hit"][0] > 100 and out["n_hit"].tolist()[1:] == [0, 0, 7]
    assert (out["depth"][1:3] == 0).all() and (out["normal"][1:3] == 0).all()
    assert (out["depth"][3] == 7).all() and (out["normal"][3] == 7).all()   # from n_views on: untouched
    for n_views in (-1, 5):
        refused = ref.raycast(dict(seq, n_views=n_views), p, origin, volume, 4, ROWS, COLS, before)
        assert refused["status"] == ref.PRS_ERR_RANGE and refused["n_skipped"] == 0
        assert all((refused[k] == 7).all() for k in ("depth", "normal", "n_hit"))
    none = ref.raycast(dict(seq, n_views=0), p, origin, volume, 4, ROWS, COLS, before)
    assert none["status"] == 0 and all((none[k] == 7).all() for k in ("depth", "normal", "n_hit"))
    # a subset of the pixels equals those pixels of the whole image
    v, u = np.array([0, 3, 19]), np.array([5, 23, 0])
    some = ref.raycast(dict(pose=pose[:1]), p, origin, volume, 1, ROWS, COLS, pixels=(v, u))
    assert some["depth"][0].tobytes() == out["depth"][0][v, u].tobytes() and some["normal"][0].tobytes() == out["normal"][0][v, u].tobytes()


def test_call_level_refusals_of_the_parameters():
    good = ref.params(CAM, voxel_size=0.05, step=0.05)
    assert not ref.refused(good, (17, 12, 9))
    nan, inf = float("nan"), float("inf")
    for bad in (dict(voxel_size=0.0), dict(voxel_size=nan), dict(step=0.0), dict(step=-1.0), dict(step=inf), dict(min_weight=nan),
                dict(range_min=-0.5), dict(range_min=3.0, range_max=2.0), dict(range_max=inf), dict(sensor_in_robot=np.full((4, 4), nan)),
                dict(step=1e-6)):                                  # 38 voxels of 5 cm hold 1.9 million steps of a micrometre
        assert ref.refused(ref.params(CAM, **dict(dict(voxel_size=0.05, step=0.05), **bad)), (17, 12, 9)), bad
    assert ref.refused(ref.params(dict(CAM, fx=nan)), (17, 12, 9)) and ref.refused(good, (17, 0, 9))
    assert not ref.refused(ref.params(CAM, voxel_size=1.0, step=2.0 ** -10), (512, 256, 256))      # exactly 2^20 steps
    assert ref.refused(ref.params(CAM, voxel_size=1.0, step=2.0 ** -10), (512, 256, 257))
