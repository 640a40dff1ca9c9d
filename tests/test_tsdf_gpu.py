"""prs_tsdf_integrate_batch_run and prs_tsdf_surface_batch_run on the device against tests/tsdf_ref.py, byte for byte: volume,
n_updates, n_skipped, status, xyz, normal, cell and the counts.

1. volume shapes below and above one brick (32 x 4 x 4) and ragged on every axis, u16 and f32 depth, a padded pitch, a batch with a
   refused sequence, pixels that are not depths
2. camera placements: inside the volume, on a single corner brick, looking away, a projection on the .5 tie, a sensor offset with a
   large rotation far from the origin
3. weights: saturation, min_weight above every weight
4. calls and outputs: two calls against one, a volume that holds data, count only, out_stride exactly full and one short, each subset
   of the optional outputs
5. refusals at the call and in the Python layer
6. a captured graph of both calls, replayed
7. the chain from the consistency filter to a PLY with normals"""
import ctypes as C

import numpy as np
import pytest

import tsdf_cases as cases
import tsdf_ref as ref
import tsdf_rig as rig_
from tsdf_rig import COLS, ROWS, SENTINEL, VS, K, Rig, origin_in_front, params_pair, scene
from srrg2_proslam_amd import _lib_tsdf, ops

pytestmark = pytest.mark.gpu
F = np.float32


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("depth_type", ["u16", "f32"])
@pytest.mark.parametrize("dims", [(1, 1, 1), (33, 5, 9), (70, 9, 6)], ids=lambda d: "%dx%dx%d" % d)
def test_shapes_types_and_pitches_in_a_batch_with_a_refused_sequence(hip_ctx, dims, depth_type, pad):
    frames = 3 + (dims[0] + pad) % 3  # 3 .. 5 images
    n_images = (frames, frames + 1, frames - 1)  # the second sequence is refused
    seqs = [scene((1, b) + dims, dims, frames, depth_type, n_images=n, index=True, pose_stride=frames + 1) for b, n in enumerate(n_images)]
    origins = [origin_in_front(dims, shift=(0.01 * b, -0.02 * b)) for b in range(3)]
    r = Rig(hip_ctx, seqs, origins, dims, depth_type, pad, out_stride=3 * dims[0] * dims[1] * dims[2])
    p, rp = params_pair(ops, depth_type, max_weight=3.0)
    marked = np.full((3, dims[2], dims[1], dims[0], 2), -7.5, F)  # the refused sequence's volume keeps these bytes
    marked[[0, 2]] = 0
    want = r.check_integrate(p, rp, marked, "integrate")
    assert [w["status"] for w in want] == [0, ref.PRS_ERR_RANGE, 0] and (want[1]["volume"] == -7.5).all()
    served = [w["n_updates"][:n] for w, n in ((want[0], frames), (want[2], frames - 1))]
    assert all(u.sum() > 0 for u in served)  # the single voxel's pixel is not a depth in every image
    surface = r.check_surface(p, rp, what="surface")
    if dims != (1, 1, 1):
        assert all(u.min() > 0 for u in served)
        assert min(s["n_total"] for s in (surface[0], surface[2])) > 30 and surface[0]["status"] == 0
        assert want[0]["volume"][..., 1].max() == 3.0 and (want[0]["volume"][..., 1] == 0).any()


def test_without_n_images_every_frame_is_served(hip_ctx):
    dims = (33, 5, 9)
    seqs = [scene((2, b), dims, 3, "f32") for b in range(2)]
    r = Rig(hip_ctx, seqs, [origin_in_front(dims)] * 2, dims)
    r.put("n_images", np.array([-5, 99], np.int32))  # not read
    p, rp = params_pair(ops)
    want = r.check_integrate(p, rp, n_images=False)
    assert all(w["status"] == 0 and w["n_updates"].min() > 0 for w in want)


def test_more_images_than_one_tile_of_poses_and_skipped_frames(hip_ctx):
    """70 images: the poses pass through LDS 32 at a time; every seventh pose is not finite, two indices lie outside pose_stride"""
    dims, frames = (33, 5, 9), 70
    seq = scene((3,), dims, frames, "u16", index=True)
    seq["pose"][::7, 5] = np.nan
    seq["frame_index"][[3, 40]] = (-1, frames)
    r = Rig(hip_ctx, [seq], [origin_in_front(dims)], dims, "u16")
    p, rp = params_pair(ops, "u16", max_weight=50.0)
    want = r.check_integrate(p, rp)[0]
    assert 10 <= want["n_skipped"] <= 12 and (want["n_updates"] == 0).sum() == want["n_skipped"]
    assert want["volume"][..., 1].max() == 50.0


# ---- 2. camera placements ---------------------------------------------------------------------------------------------------------------
PLACE_DIMS = (40, 12, 10)  # 2 x 3 x 3 bricks


def placed(pose, depth_value=0.6, frames=1):
    depth = np.full((frames, ROWS, COLS), depth_value, F)
    depth += np.linspace(0, 0.05, COLS, dtype=F)[None, None, :]
    return dict(depth=depth, pose=np.tile(np.asarray(pose, F).reshape(1, 16), (frames, 1)), n_images=frames)


def test_a_camera_inside_the_volume(hip_ctx):
    origin = origin_in_front(PLACE_DIMS, z0=-0.1)  # z from -0.1 to 0.4: the camera sits at the world's origin
    r = Rig(hip_ctx, [placed(np.eye(4), 0.3)], [origin], PLACE_DIMS, out_stride=2000)
    p, rp = params_pair(ops, range_min=0.05)
    want = r.check_integrate(p, rp)[0]
    w = want["volume"][..., 1]
    # nothing behind the camera (k < 2) or nearer than range_min (k = 2, z = 0.025); the frustum widens with every layer
    assert w[:3].max() == 0 and all(w[k].max() == 1 for k in range(3, 10)) and 50 < want["n_updates"][0] < 1500
    assert w[9].sum() > w[3].sum() and r.check_surface(p, rp)[0]["n_total"] > 10


def corner_pose():
    """to the right of and below the volume, looking down +z: the volume leaves the image at its left and upper edge and only the
    voxels of the largest i and j stay inside"""
    nx, ny, _ = PLACE_DIMS
    T = np.eye(4)
    x_last, y_last = (nx / 2 - 0.5) * VS, (ny / 2 - 0.5) * VS   # the centre of the last voxel along x and y
    # at z = 1 the image begins at x = -(cx + 0.5) / fx: the last voxel's centre lies just inside it, the one before it outside
    T[0, 3] = x_last + (K["cx"] + 0.5) / K["fx"] * 1.0 - 0.004
    T[1, 3] = y_last + (K["cy"] + 0.5) / K["fy"] * 1.0 - 0.004
    return T


def test_a_camera_that_sees_a_single_corner_brick(hip_ctx):
    origin = origin_in_front(PLACE_DIMS, z0=1.0 - VS / 2)  # the first layer's centres at z = 1
    seq = placed(corner_pose(), 0.92)  # behind the first two layers: the band ends at z = 1.07
    r = Rig(hip_ctx, [seq], [origin], PLACE_DIMS)
    p, rp = params_pair(ops)
    want = r.check_integrate(p, rp, np.full((1, 10, 12, 40, 2), 0.25, F))[0]
    k, j, i = np.nonzero(want["volume"][..., 1] != 0.25)
    assert 1 <= want["n_updates"][0] <= 6 and k.size == want["n_updates"][0]
    assert i.min() >= 32 and j.min() >= 8 and k.max() < 4                 # one brick, the last along x and y
    assert (i.max(), j.max(), k.min()) == (39, 11, 0)                        # and of it the corner voxel


def test_a_camera_that_looks_away_changes_no_byte(hip_ctx):
    T = np.eye(4)
    T[:3, :3] = cases.rot_y(np.pi)
    r = Rig(hip_ctx, [placed(T, 1.2, frames=2)], [origin_in_front(PLACE_DIMS)], PLACE_DIMS)
    p, rp = params_pair(ops)
    before = rig_.rng_of(4).normal(size=(1, 10, 12, 40, 2)).astype(F)
    want = r.check_integrate(p, rp, before)[0]
    assert want["n_updates"].tolist() == [0, 0] and want["volume"].tobytes() == before.tobytes() and want["n_skipped"] == 0


def test_a_centre_that_projects_onto_a_pixel_boundary_goes_up(hip_ctx):
    """fx = 32, cx = 11.5, voxels of 1/16 m: the centres with x = 0 project onto 11.5 + 0.5 exactly, and floorf takes column 12.
    Column 12 alone holds a depth, so those voxels are updated and their neighbours in x are not"""
    cam = dict(fx=32.0, fy=32.0, cx=11.5, cy=9.5)
    dims = (8, 6, 5)
    origin = np.array([-4.5 / 16, -3.5 / 16, 1.0, 0.0], F)  # the centres of i = 4 and of j = 3 lie on the axis
    depth = np.zeros((1, ROWS, COLS), F)
    depth[:, 10, 12] = 1.125
    r = Rig(hip_ctx, [dict(depth=depth, pose=np.eye(4, dtype=F).reshape(1, 16), n_images=1)], [origin], dims)
    p, rp = params_pair(ops, K=cam, voxel_size=1 / 16, truncation=0.25)
    want = r.check_integrate(p, rp)[0]
    k, j, i = np.nonzero(want["volume"][..., 1])
    assert set(i) == {4} and set(j) == {3} and k.size == want["n_updates"][0] == 5
    assert want["volume"][:, 3, 4, 0].tolist() == [(1.125 - (1 + (k + 0.5) / 16)) / 0.25 for k in range(5)]


def test_a_sensor_offset_with_a_large_rotation_far_from_the_origin(hip_ctx):
    rng = rig_.rng_of(5)
    dims, frames = (33, 9, 10), 3
    S = cases.random_pose(rng, 0.3)
    pose = []
    for f in range(frames):
        T = cases.random_pose(rng, 0.02).astype(np.float64)
        T[:3, 3] += (512.0, -300.0, 200.0)
        pose.append(T.astype(F).reshape(16))
    seq = scene((5, 1), dims, frames, "f32")
    seq["pose"] = np.stack(pose)
    # the volume, axis-aligned in the world, around the point 1.2 m in front of the first camera
    first = seq["pose"][0].reshape(4, 4).astype(np.float64) @ S.astype(np.float64)
    centre = first @ np.array([0, 0, 1.2, 1.0])
    origin = np.append(centre[:3] - np.array(dims) * VS / 2, 0).astype(F)
    seq["depth"] = np.where(seq["depth"] > 0, seq["depth"] - F(1.0 + dims[2] * VS / 2) + F(1.2), seq["depth"]).astype(F)
    r = Rig(hip_ctx, [seq], [origin], dims, out_stride=4000)
    p, rp = params_pair(ops, sensor_in_robot=S)
    want = r.check_integrate(p, rp)[0]
    assert want["n_updates"][0] > 300
    assert r.check_surface(p, rp)[0]["n_total"] > 30


# ---- 3. weights ----------------------------------------------------------------------------------------------------------------------------
def test_max_weight_2_with_5_frames_and_a_min_weight_above_every_weight(hip_ctx):
    dims = (33, 5, 9)
    r = Rig(hip_ctx, [scene((6,), dims, 5, "u16")], [origin_in_front(dims)], dims, "u16", out_stride=3000)
    p, rp = params_pair(ops, "u16", max_weight=2.0)
    want = r.check_integrate(p, rp)[0]
    assert want["volume"][..., 1].max() == 2.0 and want["n_updates"].min() > 100
    assert r.check_surface(p, rp)[0]["n_total"] > 30
    for min_weight, rows in ((2.0, True), (2.5, False)):
        q, rq = params_pair(ops, "u16", max_weight=2.0, min_weight=min_weight)
        s = r.check_surface(q, rq, what="min_weight %g" % min_weight)[0]
        assert (s["n_total"] > 0) == rows and s["status"] == 0


# ---- 4. calls and outputs ----------------------------------------------------------------------------------------------------------------
def test_two_calls_equal_one_call_and_a_volume_that_holds_data(hip_ctx):
    dims = (70, 9, 6)
    whole = scene((7,), dims, 4, "f32")
    halves = [dict(depth=whole["depth"][h], pose=whole["pose"][h], n_images=2) for h in (slice(0, 2), slice(2, 4))]
    p, rp = params_pair(ops, max_weight=3.0)
    one = Rig(hip_ctx, [whole], [origin_in_front(dims)], dims)
    want = one.check_integrate(p, rp)[0]
    two = Rig(hip_ctx, [halves[0]], [origin_in_front(dims)], dims)
    first = two.check_integrate(p, rp)[0]
    two.upload([halves[1]])
    second = two.check_integrate(p, rp, first["volume"][None], "the second half")[0]
    assert second["volume"].tobytes() == want["volume"].tobytes() == one.get("volume")[0].tobytes()
    assert first["n_updates"].tolist() + second["n_updates"].tolist() == want["n_updates"].tolist()
    # another sequence's images into that volume
    two.upload([scene((7, 1), dims, 2, "f32")])
    third = two.check_integrate(p, rp, second["volume"][None], "another sequence's images")[0]
    assert third["volume"].tobytes() != second["volume"].tobytes() and third["volume"][..., 1].max() == 3.0


@pytest.fixture(scope="module")
def fused(hip_ctx):
    """a batch of two fused volumes and the crossings the restatement finds in them"""
    dims = (33, 5, 9)
    r = Rig(hip_ctx, [scene((8, b), dims, 3, "f32") for b in range(2)], [origin_in_front(dims, shift=(0.0, 0.01 * b)) for b in range(2)], dims,
            out_stride=1200)
    p, rp = params_pair(ops)
    want = r.check_integrate(p, rp)
    volume = np.stack([w["volume"] for w in want])
    totals = [ref.surface(v, rp, o, 0, count_only=True)["n_total"] for v, o in zip(volume, r.origins)]
    assert 30 < min(totals) < max(totals) < 1200
    return r, p, rp, volume, totals


def test_count_only_and_out_stride_exactly_full_and_one_short(fused):
    r, p, rp, volume, totals = fused
    count = r.check_surface(p, rp, volume, outputs=(), what="count only")
    assert [c["n_total"] for c in count] == totals and [c["n_out"] for c in count] == [0, 0]
    full = r.check_surface(p, rp, volume, out_stride=max(totals), what="exactly full")
    assert [f["status"] for f in full] == [0, 0] and [f["n_out"] for f in full] == totals
    short = r.check_surface(p, rp, volume, out_stride=max(totals) - 1, what="one short")
    worst = int(np.argmax(totals))
    assert short[worst]["status"] == ref.PRS_ERR_CAPACITY and short[1 - worst]["status"] == 0
    assert short[worst]["n_out"] == max(totals) - 1 and short[worst]["n_total"] == max(totals)
    n = max(totals) - 1
    assert short[worst]["xyz"].tobytes() == full[worst]["xyz"][:n].tobytes() and short[worst]["cell"].tobytes() == full[worst]["cell"][:n].tobytes()
    tiny = r.check_surface(p, rp, volume, out_stride=1, what="one row")
    assert [t["n_out"] for t in tiny] == [1, 1] and [t["n_total"] for t in tiny] == totals


@pytest.mark.parametrize("outputs", [("xyz",), ("xyz", "normal"), ("xyz", "cell"), ("xyz", "normal", "cell")], ids="+".join)
def test_each_subset_of_the_optional_surface_outputs(fused, outputs):
    r, p, rp, volume, _ = fused
    r.check_surface(p, rp, volume, outputs=outputs)


def test_integrate_without_n_updates(fused):
    r, p, rp, _, _ = fused
    r.check_integrate(p, rp, n_updates=False)


def test_the_volume_batch_class(hip_ctx, tmp_path):
    import torch
    from srrg2_proslam_amd import formats
    dims, frames = (33, 5, 9), 3
    seqs = [scene((9, b), dims, frames, "u16") for b in range(2)]
    origins = np.stack([origin_in_front(dims)] * 2)
    p, rp = params_pair(ops, "u16")
    vb = ops.TsdfVolumeBatch(2, *dims, frames, ROWS, COLS, out_stride=1500)
    vb.origin.copy_(torch.from_numpy(origins))
    depth = torch.from_numpy(np.stack([s["depth"] for s in seqs])).cuda()
    pose = torch.from_numpy(np.stack([s["pose"] for s in seqs])).cuda()
    assert vb.integrate(hip_ctx, p, depth, pose) is vb.volume
    vb.integrate(hip_ctx, p, depth, pose, torch.tensor([1, 0], dtype=torch.int32, device="cuda"))
    xyz, normal, n_out = vb.surface(hip_ctx, p)
    hip_ctx.synchronize()
    for b, s in enumerate(seqs):
        once = ref.integrate(dict(s, n_images=None), rp, origins[b], np.zeros((dims[2], dims[1], dims[0], 2), F))
        twice = ref.integrate(dict(s, n_images=(1, 0)[b]), rp, origins[b], once["volume"])
        assert vb.volume[b].cpu().numpy().tobytes() == twice["volume"].tobytes()
        assert vb.n_updates[b].cpu().tolist() == twice["n_updates"].tolist() and vb.status.cpu().tolist() == [0, 0]
        want = ref.surface(twice["volume"], rp, origins[b], 1500)
        n = int(n_out[b].item())
        assert n == want["n_out"] > 30 and int(vb.n_total[b].item()) == n and int(vb.surface_status[b].item()) == 0
        assert xyz[b].cpu().numpy().tobytes() == want["xyz"].tobytes() and normal[b].cpu().numpy().tobytes() == want["normal"].tobytes()
        assert vb.cell[b].cpu().numpy().tobytes() == want["cell"].tobytes()
    assert vb.count(hip_ctx, p) is vb.n_total
    vb.clear()
    vb.surface(hip_ctx, p)
    hip_ctx.synchronize()
    assert vb.n_total.cpu().tolist() == [0, 0] and not vb.volume.any().item()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_call_level_refusals_write_nothing(fused):
    r, p, rp, volume, _ = fused
    lib, ctx = _lib_tsdf.load(), r.ctx._h
    outputs = ("volume", "n_updates", "n_skipped", "status", "xyz", "normal", "cell", "n_out", "n_total", "surface_status")
    r.fill_outputs(outputs)

    def run(d, q=None, entry="prs_tsdf_integrate_batch_run"):
        q = p if q is None else q
        return getattr(lib, entry)(ctx, C.byref(q) if q != "null" else None, C.byref(d) if d is not None else None)

    def surf(d, q=None):
        return run(d, q, "prs_tsdf_surface_batch_run")

    def changed(**fields):
        q = ops.tsdf_params(K, depth_type="f32", voxel_size=VS, truncation=rig_.TRUNC)
        for k, v in fields.items():
            setattr(q, k, v)
        return q

    D, S = r.descriptor, r.surface_descriptor
    nan, inf = float("nan"), float("inf")
    # PRS_ERR_NULL
    assert run(None) == -1 and run(D(), "null") == -1 and surf(None) == -1 and surf(S(), "null") == -1
    for field in ("depth", "pose", "origin", "volume", "n_skipped", "status", "workspace"):
        d = D()
        setattr(d, field, None)
        assert run(d) == -1, field
    for field in ("origin", "volume", "n_out", "n_total", "status", "workspace"):
        d = S()
        setattr(d, field, None)
        assert surf(d) == -1, field
    for outputs_ in (("normal",), ("cell",), ("normal", "cell")):
        assert surf(S(outputs=outputs_)) == -1, outputs_
    # PRS_ERR_RANGE
    for field, value in (("batch", 0), ("frames", 0), ("rows", 0), ("cols", -1), ("pose_stride", 0), ("nx", 0), ("ny", -3), ("nz", 0),
                         ("pitch", 4 * COLS - 4), ("pitch", 4 * COLS + 2), ("pitch", -4 * COLS)):
        d = D()
        setattr(d, field, value)
        assert run(d) == ref.PRS_ERR_RANGE, (field, value)
    for field, value in (("batch", 0), ("nx", 0), ("ny", 0), ("nz", -1), ("out_stride", 0), ("out_stride", -1)):
        d = S()
        setattr(d, field, value)
        assert surf(d) == ref.PRS_ERR_RANGE, (field, value)
    for field, value in (("voxel_size", 0.0), ("voxel_size", -VS), ("voxel_size", nan), ("voxel_size", inf), ("truncation", 0.0),
                         ("truncation", -1.0), ("truncation", nan), ("max_weight", 0.5), ("max_weight", nan), ("max_weight", inf),
                         ("depth_scaling_factor_to_meters", 0.0), ("depth_scaling_factor_to_meters", -1.0),
                         ("depth_scaling_factor_to_meters", nan), ("fx", inf), ("fy", nan), ("cx", -inf), ("cy", nan), ("range_min", -1.0),
                         ("range_min", 11.0), ("range_min", nan), ("range_max", inf)):
        assert run(D(), changed(**{field: value})) == ref.PRS_ERR_RANGE, (field, value)
    q = changed()
    q.sensor_in_robot[14] = nan
    assert run(D(), q) == ref.PRS_ERR_RANGE
    for field, value in (("voxel_size", 0.0), ("voxel_size", nan), ("voxel_size", inf), ("min_weight", nan), ("min_weight", inf)):
        assert surf(S(), changed(**{field: value})) == ref.PRS_ERR_RANGE, (field, value)
    # what a call does not read does not refuse it: min_weight for integrate, the camera and the truncation for the surface
    # (these two run: the sentinel check below looks at what the refusals left, so they come last)
    # PRS_ERR_UNSUPPORTED
    for value in (2, -1):
        assert run(D(), changed(depth_type=value)) == -5, value
    for field, step in (("depth", 2), ("volume", 8), ("volume", 4), ("workspace", 8), ("n_images", 2), ("pose", 2), ("origin", 2),
                        ("n_updates", 1), ("n_skipped", 2), ("status", 2)):
        d = D()
        setattr(d, field, getattr(d, field) + step)
        assert run(d) == -5, field
    for field, step in (("volume", 8), ("xyz", 8), ("normal", 4), ("workspace", 8), ("origin", 2), ("cell", 2), ("n_out", 1), ("n_total", 2),
                        ("status", 2)):
        d = S()
        setattr(d, field, getattr(d, field) + step)
        assert surf(d) == -5, field
    # more voxels than (2^31 - 1) / 3, more pixels or images than 2^31 - 1, more bricks than one launch takes
    for nx, ny, nz in ((1024, 1024, 683), (1 << 16, 1 << 16, 1 << 16), (1 << 30, 1, 1)):
        d, s = D(), S()
        d.nx, d.ny, d.nz = s.nx, s.ny, s.nz = nx, ny, nz
        assert run(d) == -5 and surf(s) == -5, (nx, ny, nz)
    d = D()
    d.nx, d.ny, d.nz = 1, 1 << 14, 1 << 14  # 2^28 voxels in 2^24 bricks of one column
    assert run(d) == -5
    for b, f, rows, cols in ((1 << 16, 1 << 15, 1, 1), (1, 1, 1 << 16, 1 << 15)):
        d = D()
        d.batch, d.frames, d.rows, d.cols, d.pitch = b, f, rows, cols, 4 * cols
        assert run(d) == -5, (b, f, rows, cols)
    r.ctx.synchronize()
    for name in outputs:
        assert (r.get(name).view(np.uint8) == SENTINEL).all(), name
    assert b"prs_tsdf_integrate_batch_run" in lib.prs_last_error(ctx)
    r.put("volume", volume)
    assert run(D(), changed(min_weight=nan)) == 0 and surf(S(), changed(truncation=nan, fx=nan, max_weight=0.0, depth_type=7)) == 0
    r.ctx.synchronize()


def test_the_python_layer_refuses_what_it_cannot_describe(hip_ctx):
    import torch
    vb = ops.TsdfVolumeBatch(2, 5, 4, 3, 2, 5, 6, out_stride=10)
    p = ops.tsdf_params(K, depth_type="f32")
    ok = torch.zeros((2, 2, 5, 6), dtype=torch.float32, device="cuda")
    pose = torch.zeros((2, 2, 16), dtype=torch.float32, device="cuda")
    vb.descriptor(p, ok, pose)
    vb.descriptor(p, torch.zeros((2, 2, 5, 8), dtype=torch.float32, device="cuda")[..., :6], pose)
    for bad in (ok.to(torch.float64), ok[..., :5], ok[:, :, :4], ok.transpose(2, 3).contiguous().transpose(2, 3), ok[:, :1].expand(2, 2, 5, 6),
                torch.zeros((2, 2, 5, 6), dtype=torch.uint16, device="cuda")):
        with pytest.raises(ValueError):
            vb.descriptor(p, bad, pose)
    with pytest.raises(ValueError):
        vb.descriptor(ops.tsdf_params(K, depth_type="u16"), ok, pose)
    for bad in (pose[:1], pose[..., :12], pose.reshape(2, 2, 4, 4), pose.to(torch.float64)):
        with pytest.raises(ValueError):
            vb.descriptor(p, ok, bad)
    with pytest.raises(ValueError):
        vb.descriptor(p, ok, pose, n_images=torch.zeros((3,), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        vb.descriptor(p, ok, pose, frame_index=torch.zeros((2, 3), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.TsdfVolumeBatch(2, 5, 4, 3, 2, 5, 6).surface_descriptor()  # no rows
    ops.TsdfVolumeBatch(2, 5, 4, 3, 2, 5, 6).surface_descriptor(count_only=True)
    for bad in (dict(batch=0), dict(nx=0), dict(ny=0), dict(nz=-1), dict(frames=0), dict(rows=0), dict(cols=0), dict(out_stride=0),
                dict(nx=1024, ny=1024, nz=683), dict(batch=1 << 16, frames=1 << 15)):
        with pytest.raises(ValueError):
            ops.TsdfVolumeBatch(**dict(dict(batch=1, nx=2, ny=2, nz=2, frames=1, rows=2, cols=2), **bad))


# ---- 6. capture --------------------------------------------------------------------------------------------------------------------------
def test_integrate_and_surface_in_one_captured_graph_replayed_twice(hip_ctx):
    import torch
    ctx = hip_ctx
    dims = (33, 5, 9)
    seqs = [scene((10, b), dims, 3, "f32", n_images=n) for b, n in enumerate((3, 2))]
    r = Rig(ctx, seqs, [origin_in_front(dims)] * 2, dims, out_stride=1500)
    p, rp = params_pair(ops)
    empty = np.zeros((2, dims[2], dims[1], dims[0], 2), F)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        assert r.integrate(p) == 0 and r.surface(p) == 0  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            assert r.integrate(p) == 0 and r.surface(p) == 0
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    torch.cuda.synchronize()

    def replay_and_compare(what):
        r.put("volume", empty)
        r.fill_outputs(("n_updates", "n_skipped", "status", "xyz", "normal", "cell", "n_out", "n_total", "surface_status"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = r.expected_integrate(rp, empty)
        r.compare_integrate(want, what)
        got = {k: r.get(k) for k in ("xyz", "normal", "cell", "n_out", "n_total", "surface_status")}
        for b, w in enumerate(want):
            before = dict(xyz=rig_.sentinel((1500, 4), F), normal=rig_.sentinel((1500, 4), F), cell=rig_.sentinel((1500,), np.int32))
            sw = ref.surface(w["volume"], rp, r.origins[b], 1500, before)
            assert (int(got["surface_status"][b]), int(got["n_out"][b]), int(got["n_total"][b])) == (sw["status"], sw["n_out"], sw["n_total"])
            for name in ("xyz", "normal", "cell"):
                assert got[name][b].tobytes() == sw[name].tobytes(), (what, b, name)
        return want

    for replay in range(2):
        want = replay_and_compare("replay %d" % replay)
        assert [w["status"] for w in want] == [0, 0]
    # and on other images, a sequence of which is refused now
    r.upload([scene((10, b, 1), dims, 3, "f32", n_images=n) for b, n in enumerate((1, 4))])
    want = replay_and_compare("replay on other images")
    assert [w["status"] for w in want] == [0, ref.PRS_ERR_RANGE]


# ---- 7. the chain ------------------------------------------------------------------------------------------------------------------------
def test_consistency_filter_integrate_surface_ply(hip_ctx, tmp_path):
    """the consistency filter's out is the depth the fusion reads, in place; the surface goes to a PLY with normals, which is read
    back.  Everything equals the restatements chained on the CPU"""
    import torch

    import depth_consistency_ref as cref
    from srrg2_proslam_amd import formats
    B, frames, dims = 1, 4, (33, 9, 9)
    seq = scene((11,), dims, frames, "f32", bad=True)
    ckw = dict(range_min=0.1, range_max=10.0, scale=1.0)
    fkw = dict(window=2, stride=1, max_rel_diff=0.1, min_support=1, max_violation=1)
    filtered = cref.depth_consistency(dict(depth=seq["depth"], pose=seq["pose"]), cref.params(K, **fkw, **ckw))
    want_depth = np.stack([i["out"] for i in filtered["results"]])
    p, rp = params_pair(ops)
    origin = origin_in_front(dims)
    want = ref.integrate(dict(seq, depth=want_depth), rp, origin, np.zeros((dims[2], dims[1], dims[0], 2), F))
    want_surface = ref.surface(want["volume"], rp, origin, 4000)
    n = want_surface["n_out"]
    assert 50 < n == want_surface["n_total"] and 0 < (want_depth > 0).sum() < (seq["depth"] > 0).sum()

    dev = torch.device("cuda", 0)
    t_pose = torch.from_numpy(seq["pose"]).to(dev).unsqueeze(0)
    dcb = ops.DepthConsistencyBatch(B, frames, ROWS, COLS, 2, "f32")
    out = dcb.run(hip_ctx, ops.depth_consistency_params(K, depth_type="f32", **fkw, **ckw), torch.from_numpy(seq["depth"]).to(dev).unsqueeze(0), t_pose)
    vb = ops.TsdfVolumeBatch(B, *dims, frames, ROWS, COLS, out_stride=4000)
    vb.origin.copy_(torch.from_numpy(origin[None]))
    vb.integrate(hip_ctx, p, out, t_pose)
    xyz, normal, n_out = vb.surface(hip_ctx, p)
    hip_ctx.synchronize()
    assert out.cpu().numpy().tobytes() == want_depth[None].tobytes()
    assert vb.volume.cpu().numpy().tobytes() == want["volume"][None].tobytes() and vb.n_updates.cpu().tolist() == [want["n_updates"].tolist()]
    assert int(n_out[0].item()) == n
    got_xyz, got_normal = xyz[0, :n].cpu().numpy(), normal[0, :n].cpu().numpy()
    assert got_xyz.tobytes() == want_surface["xyz"][:n].tobytes() and got_normal.tobytes() == want_surface["normal"][:n].tobytes()
    path = str(tmp_path / "surface.ply")
    formats.write_ply(path, got_xyz, normals=got_normal)
    head, body = open(path, "rb").read().split(b"end_header\n")
    assert b"element vertex %d\n" % n in head and head.decode().split("\n")[3:-1] == ["property float %s" % a for a in ("x", "y", "z", "nx", "ny", "nz")]
    rows = np.frombuffer(body, F).reshape(n, 6)
    assert rows[:, :3].tobytes() == want_surface["xyz"][:n, :3].tobytes() and rows[:, 3:].tobytes() == want_surface["normal"][:n, :3].tobytes()
