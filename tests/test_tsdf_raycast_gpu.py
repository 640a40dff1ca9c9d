"""prs_tsdf_raycast_batch_run on the device against tests/tsdf_raycast_ref.py, byte for byte: depth, normal, n_hit, n_skipped, status,
and the sentinel wherever the rule writes nothing.

1. base: batches of three volumes, permuted views out of a longer pose array
2. image shapes: one pixel, one row, sizes that are no multiple of the tile, a padded pitch
3. axis-parallel rays, inside and outside the slab
4. camera placements and ranges
5. steps, unobserved space, volumes without a surface
6. view rules and optional pointers
7. refusals at the call and in the Python layer
8. a captured graph, replayed
9. the sphere scene, and the chain from the integrator through the raycast to the dense cloud"""
import ctypes as C

import numpy as np
import pytest

import tsdf_cases as cases
import tsdf_raycast_ref as ref
import tsdf_raycast_rig as rig_
import tsdf_ref
import tsdf_rig
from tsdf_raycast_rig import Rig, fused, normals_of, params_pair, views_of
from tsdf_rig import COLS, ROWS, SENTINEL, VS, K
from srrg2_proslam_amd import _lib_tsdf_raycast, ops

pytestmark = pytest.mark.gpu
F = np.float32
DIMS = (17, 12, 9)


def at(x=0.0, y=0.0, z=0.0, yaw=0.0):
    T = np.eye(4)
    T[:3, :3] = cases.rot_y(yaw)
    T[:3, 3] = (x, y, z)
    return T.astype(F).reshape(1, 16)


def one(ctx, pose, dims=DIMS, key=(3,), volume=None, **kw):
    """a rig of one volume and one view from `pose` [1, 16]"""
    vol, origin = fused(key + dims, dims)
    return Rig(ctx, [vol if volume is None else volume], [origin], [dict(pose=pose, n_views=1)], 1, **kw)


# ---- 1. base ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,key,hits,normals", [((17, 12, 9), 1, 100, 60), ((33, 5, 9), 2, 50, 15)], ids=["17x12x9", "33x5x9"])
def test_a_batch_of_three_volumes_with_permuted_views(hip_ctx, dims, key, hits, normals):
    views = 3
    made = [fused((key, b) + dims, dims) for b in range(3)]
    seqs = [views_of((key, b) + dims, views, views + 1, index=True) for b in range(3)]
    r = Rig(hip_ctx, [m[0] for m in made], [m[1] for m in made], seqs, views)
    p, rp = params_pair(ops)
    want = r.check(p, rp, "base")
    for w in want:
        assert w["status"] == 0 and w["n_skipped"] == 0
        assert w["n_hit"].min() > hits and normals_of(w).min() > normals, (w["n_hit"], normals_of(w))


# ---- 2. image shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,pad", [(1, 1, 0), (1, 70, 0), (17, 9, 0), (20, 24, 3)], ids=["1x1", "1x70", "17x9", "20x24+3"])
def test_image_shapes_and_a_padded_pitch(hip_ctx, rows, cols, pad):
    views = 2
    made = [fused((1, b) + DIMS, DIMS) for b in range(2)]
    seqs = [views_of((4, b), views) for b in range(2)]
    r = Rig(hip_ctx, [m[0] for m in made], [m[1] for m in made], seqs, views, rows, cols, pad)
    camera = dict(K, cx=(cols - 1) / 2, cy=(rows - 1) / 2) if rows * cols > 1 else dict(K, cx=0.0, cy=0.0)
    p, rp = params_pair(ops, camera)
    want = r.check(p, rp, "shape")
    assert all(w["n_hit"].min() > 0 for w in want)


# ---- 3. axis-parallel rays -------------------------------------------------------------------------------------------------------------
AXIS = dict(fx=30, fy=29, cx=12.0, cy=10.0)


def test_rays_parallel_to_an_axis_inside_and_outside_the_slab(hip_ctx):
    p, rp = params_pair(ops, AXIS)
    r = one(hip_ctx, at())
    T = ref.view_transform(r.seqs[0], 0, rp)
    v, u = np.meshgrid(np.arange(ROWS), np.arange(COLS), indexing="ij")
    dw0 = (T[0, 0] * ((u.astype(F) - rp["cx"]) / rp["fx"]) + T[0, 1] * ((v.astype(F) - rp["cy"]) / rp["fy"])) + T[0, 2] * F(1)
    assert (dw0[:, 12] == 0).all() and (dw0 != 0).sum() == ROWS * (COLS - 1)  # column 12 takes the dw == 0 branch on x, row 10 on y
    inside = r.check(p, rp, "inside")[0]
    assert (inside["depth"][0][:, 12] > 0).sum() > 5 and (inside["depth"][0][10] > 0).sum() > 5
    r = one(hip_ctx, at(x=0.6))  # the box ends at x = 0.4: the rays with dw0 == 0 miss, those that lean back still enter
    outside = r.check(p, rp, "outside")[0]
    assert (outside["depth"][0][:, 12:] == 0).all() and outside["n_hit"][0] > 0


# ---- 4. placements ---------------------------------------------------------------------------------------------------------------------
def test_a_camera_inside_the_volume_in_front_of_the_surface(hip_ctx):
    p, rp = params_pair(ops)
    want = one(hip_ctx, at(z=1.05)).check(p, rp)[0]  # the voxel centres start at z = 1.025, the surface runs about z = 1.2
    assert want["n_hit"][0] > 100 and normals_of(want)[0] > 50


def test_a_camera_behind_the_surface_hits_nothing(hip_ctx):
    p, rp = params_pair(ops)
    # looks back at the volume from behind the half without the depth step (from behind the step the free space beside the nearer
    # surface is seen through its side, and the rule hits there): every ray that meets the band meets negative values first
    want = one(hip_ctx, at(x=-0.2, z=1.6, yaw=np.pi)).check(p, rp)[0]
    front = ref.raycast(dict(pose=at(x=-0.2)), rp, fused((3,) + DIMS, DIMS)[1], fused((3,) + DIMS, DIMS)[0], 1, ROWS, COLS)
    assert front["n_hit"][0] > 100  # the same column of the volume holds a surface
    assert want["n_hit"][0] == 0 and (want["depth"] == 0).all() and (want["normal"] == 0).all()


def test_a_camera_that_looks_away_and_rays_that_miss_the_box(hip_ctx):
    p, rp = params_pair(ops)
    for pose in (at(yaw=np.pi), at(x=5.0), at(y=-4.0, z=1.2)):
        want = one(hip_ctx, pose).check(p, rp)[0]
        assert want["status"] == 0 and want["n_hit"][0] == 0 and (want["depth"] == 0).all() and (want["normal"] == 0).all()


def test_a_sensor_that_is_not_at_the_robots_origin(hip_ctx):
    S = np.eye(4)
    S[:3, :3] = cases.rot_y(0.15)
    S[:3, 3] = (0.03, -0.02, 0.05)
    p, rp = params_pair(ops, sensor_in_robot=S.astype(F))
    r = one(hip_ctx, at(x=-0.1, yaw=-0.1))
    want = r.check(p, rp)[0]
    plain = ref.raycast(r.seqs[0], params_pair(ops)[1], r.origins[0], r.volumes[0], 1, ROWS, COLS)
    assert want["n_hit"][0] > 100 and want["depth"].tobytes() != plain["depth"].tobytes()


def test_ranges_that_begin_inside_the_volume_and_end_in_front_of_the_surface(hip_ctx):
    r = one(hip_ctx, at())
    p, rp = params_pair(ops)
    whole = r.check(p, rp)[0]
    p, rp = params_pair(ops, range_min=1.2)   # some rays now start behind the surface
    inside = r.check(p, rp)[0]
    assert 0 < inside["n_hit"][0] < whole["n_hit"][0] and inside["depth"][inside["depth"] > 0].min() >= F(1.2)
    p, rp = params_pair(ops, range_max=1.1)
    front = r.check(p, rp)[0]
    assert front["n_hit"][0] == 0
    p, rp = params_pair(ops, range_min=1.25, range_max=1.25)  # one sample a ray: never a hit
    assert r.check(p, rp)[0]["n_hit"][0] == 0


# ---- 5. steps, weights, empty volumes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0.5, 1.5])
def test_steps_of_half_a_voxel_and_of_one_and_a_half(hip_ctx, factor):
    made = [fused((1, b) + DIMS, DIMS) for b in range(2)]
    r = Rig(hip_ctx, [m[0] for m in made], [m[1] for m in made], [views_of((5, b), 2) for b in range(2)], 2)
    p, rp = params_pair(ops, step=VS * factor)
    assert all(w["n_hit"].min() > 100 for w in r.check(p, rp))


def test_min_weight_2_on_weights_of_1_and_2(hip_ctx):
    vol, origin = fused((6,) + DIMS, DIMS, 2, True)  # two images with pixels that are not depths
    assert set(np.unique(vol[..., 1])) == {0.0, 1.0, 2.0}
    r = Rig(hip_ctx, [vol], [origin], [views_of((6,), 2)], 2)
    all_ = r.check(*params_pair(ops))[0]
    two = r.check(*params_pair(ops, min_weight=2.0))[0]
    none = r.check(*params_pair(ops, min_weight=2.5))[0]
    assert 0 < two["n_hit"].max() and (two["n_hit"] < all_["n_hit"]).all() and (none["n_hit"] == 0).all()


def test_volumes_without_a_surface(hip_ctx):
    p, rp = params_pair(ops)
    zero = one(hip_ctx, at(), volume=np.zeros((9, 12, 17, 2), F)).check(p, rp)[0]
    assert zero["n_hit"][0] == 0 and (zero["depth"] == 0).all()
    dims = (17, 1, 9)
    flat = one(hip_ctx, at(), dims=dims).check(p, rp)[0]  # no cell along y
    assert fused((3,) + dims, dims)[0][..., 1].max() >= 1 and flat["n_hit"][0] == 0 and (flat["depth"] == 0).all()


# ---- 6. view rules and optional pointers -----------------------------------------------------------------------------------------------
def test_skipped_views_a_refused_sequence_and_views_from_n_views_on(hip_ctx):
    views = 4
    made = [fused((1, b) + DIMS, DIMS) for b in range(3)]
    seqs = [views_of((7, b), views, views + 1, index=True, n_views=n) for b, n in enumerate((1, 7, views))]
    seqs[2]["view_index"][1] = views + 1      # outside pose_stride
    seqs[2]["view_index"][3] = -1
    seqs[2]["pose"][seqs[2]["view_index"][2], 9] = np.nan
    seqs[0]["pose"][seqs[0]["view_index"][0], 14] = np.nan  # the bottom row is not looked at
    r = Rig(hip_ctx, [m[0] for m in made], [m[1] for m in made], seqs, views)
    want = r.check(*params_pair(ops))
    assert [w["status"] for w in want] == [0, ref.PRS_ERR_RANGE, 0] and [w["n_skipped"] for w in want] == [0, 0, 3]
    assert want[0]["n_hit"][0] > 100 and (want[0]["n_hit"][1:].view(np.uint8) == SENTINEL).all()
    assert (want[1]["depth"].view(np.uint8) == SENTINEL).all() and (want[1]["n_hit"].view(np.uint8) == SENTINEL).all()
    assert want[2]["n_hit"].tolist()[1:] == [0, 0, 0] and (want[2]["depth"][1:] == 0).all() and (want[2]["normal"][1:] == 0).all()
    for n_views in ((0, 0, 0), (-1, views + 1, views)):
        for s, n in zip(seqs, n_views):
            s["n_views"] = n
        r.upload(seqs)
        r.check(*params_pair(ops), what="n_views %s" % (n_views,))


@pytest.mark.parametrize("off", ["normal", "n_hit", "n_views", "view_index"])
def test_each_optional_pointer_left_out(hip_ctx, off):
    views = 2
    made = [fused((1, b) + DIMS, DIMS) for b in range(2)]
    seqs = [views_of((8, b), views, views + 1, index=True, n_views=n) for b, n in enumerate((1, 2))]
    r = Rig(hip_ctx, [m[0] for m in made], [m[1] for m in made], seqs, views)
    if off == "n_views":
        r.put("n_views", np.array([-5, 99], np.int32))  # not read
    want = r.check(*params_pair(ops), what=off, **{off: False})
    assert all(w["status"] == 0 for w in want) and (want[1]["depth"] > 0).reshape(views, -1).sum(1).min() > 100
    served = [(w["depth"].reshape(views, -1).view(np.uint8) != SENTINEL).any(1).tolist() for w in want]
    assert served == ([[True, True]] * 2 if off == "n_views" else [[True, False], [True, True]])


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_call_level_refusals_write_nothing(hip_ctx):
    made = [fused((1, b) + DIMS, DIMS) for b in range(2)]
    r = Rig(hip_ctx, [m[0] for m in made], [m[1] for m in made], [views_of((8, b), 2, 3, index=True) for b in range(2)], 2)
    lib, ctx = _lib_tsdf_raycast.load(), r.ctx._h
    p, _ = params_pair(ops)
    r.fill_outputs()

    def run(d, q=None):
        q = p if q is None else q
        return lib.prs_tsdf_raycast_batch_run(ctx, C.byref(q) if q != "null" else None, C.byref(d) if d is not None else None)

    def changed(**fields):
        q, _ = params_pair(ops)
        for k, v in fields.items():
            setattr(q, k, v)
        return q

    D = r.descriptor
    nan, inf = float("nan"), float("inf")
    # PRS_ERR_NULL
    assert run(None) == -1 and run(D(), "null") == -1
    for field in ("origin", "volume", "pose", "depth", "n_skipped", "status", "workspace"):
        d = D()
        setattr(d, field, None)
        assert run(d) == -1, field
    # PRS_ERR_RANGE
    for field, value in (("batch", 0), ("views", 0), ("rows", 0), ("cols", -1), ("pose_stride", 0), ("nx", 0), ("ny", -3), ("nz", 0),
                         ("pitch", 4 * COLS - 4), ("pitch", 4 * COLS + 2), ("pitch", -4 * COLS)):
        d = D()
        setattr(d, field, value)
        assert run(d) == ref.PRS_ERR_RANGE, (field, value)
    for field, value in (("voxel_size", 0.0), ("voxel_size", -VS), ("voxel_size", nan), ("voxel_size", inf), ("step", 0.0), ("step", -VS),
                         ("step", nan), ("step", inf), ("min_weight", nan), ("min_weight", inf), ("fx", inf), ("fy", nan), ("cx", -inf),
                         ("cy", nan), ("range_min", -1.0), ("range_min", 11.0), ("range_min", nan), ("range_max", inf),
                         ("step", 1e-6)):  # 38 voxels of 5 cm hold 1.9 million steps of a micrometre
        assert run(D(), changed(**{field: value})) == ref.PRS_ERR_RANGE, (field, value)
    q = changed()
    q.sensor_in_robot[14] = nan
    assert run(D(), q) == ref.PRS_ERR_RANGE
    d = D()
    d.nx, d.ny, d.nz = 512, 256, 257            # 1025 voxels of 1 m hold more than 2^20 steps of 2^-10 m
    assert run(d, changed(voxel_size=1.0, step=2.0 ** -10)) == ref.PRS_ERR_RANGE
    # PRS_ERR_UNSUPPORTED
    for field, step in (("volume", 8), ("volume", 4), ("normal", 8), ("normal", 4), ("workspace", 8), ("depth", 2), ("origin", 2), ("pose", 2),
                        ("view_index", 2), ("n_views", 1), ("n_hit", 2), ("n_skipped", 2), ("status", 2)):
        d = D()
        setattr(d, field, getattr(d, field) + step)
        assert run(d) == -5, field
    for nx, ny, nz in ((1024, 1024, 683), (1 << 16, 1 << 16, 1 << 16), (1 << 30, 1, 1)):
        d = D()
        d.nx, d.ny, d.nz = nx, ny, nz
        assert run(d, changed(step=1e4)) == -5, (nx, ny, nz)
    for b, f, rows, cols in ((1 << 16, 1 << 15, 1, 1), (1, 1, 1 << 16, 1 << 15)):
        d = D()
        d.batch, d.views, d.rows, d.cols, d.pitch = b, f, rows, cols, 4 * cols
        assert run(d) == -5, (b, f, rows, cols)
    d = D()
    d.rows, d.cols, d.pitch = 1, 1 << 28, 1 << 30  # 2^24 tiles: more workgroups than one launch holds
    assert run(d) == -5
    r.ctx.synchronize()
    for name in rig_.OUTPUTS:
        assert (r.get(name).view(np.uint8) == SENTINEL).all(), name
    assert b"prs_tsdf_raycast_batch_run" in lib.prs_last_error(ctx)
    assert run(D()) == 0
    r.ctx.synchronize()


def test_the_python_layer_refuses_what_it_cannot_describe(hip_ctx):
    import torch
    vb = ops.TsdfVolumeBatch(2, 5, 4, 3, 2, 5, 6)
    rb = ops.TsdfRaycastBatch(hip_ctx, vb, 3, 5, 6)
    assert tuple(rb.depth.shape) == (2, 3, 5, 6) and tuple(rb.normal.shape) == (2, 3, 5, 6, 4) and tuple(rb.n_hit.shape) == (2, 3)
    pose = torch.zeros((2, 4, 16), dtype=torch.float32, device="cuda")
    d = rb.descriptor(pose)
    assert (d.pose_stride, d.pitch, d.nx, d.ny, d.nz, d.volume, d.origin) == (4, 24, 5, 4, 3, vb.volume.data_ptr(), vb.origin.data_ptr())
    for bad in (pose[:1], pose[..., :12], pose.reshape(2, 4, 4, 4), pose.to(torch.float64)):
        with pytest.raises(ValueError):
            rb.descriptor(bad)
    with pytest.raises(ValueError):
        rb.descriptor(pose, n_views=torch.zeros((3,), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        rb.descriptor(pose, view_index=torch.zeros((2, 2), dtype=torch.int32, device="cuda"))
    for bad in (dict(views=0), dict(rows=0), dict(cols=-1), dict(rows=1 << 16, cols=1 << 15)):
        with pytest.raises(ValueError):
            ops.TsdfRaycastBatch(hip_ctx, vb, **dict(dict(views=1, rows=2, cols=2), **bad))
    with pytest.raises(ValueError):
        rb.run(ops.tsdf_raycast_params(K, voxel_size=1.0, step=1e-6), pose)


# ---- 8. capture ------------------------------------------------------------------------------------------------------------------------
def test_a_captured_graph_replayed_twice_equals_the_eager_bytes(hip_ctx):
    import torch
    ctx = hip_ctx
    made = [fused((1, b) + DIMS, DIMS) for b in range(2)]
    seqs = [views_of((10, b), 3, n_views=n) for b, n in enumerate((3, 2))]
    r = Rig(ctx, [m[0] for m in made], [m[1] for m in made], seqs, 3)
    p, rp = params_pair(ops)
    r.check(p, rp, "eager")
    eager = {k: r.get(k).tobytes() for k in rig_.OUTPUTS}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        assert r.run(p) == 0  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            assert r.run(p) == 0
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    torch.cuda.synchronize()
    for replay in range(2):
        r.fill_outputs()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert {k: r.get(k).tobytes() for k in rig_.OUTPUTS} == eager, replay
    # and on other views, a sequence of which is refused now
    r.upload([views_of((10, b, 1), 3, n_views=n) for b, n in enumerate((1, 4))])
    r.fill_outputs()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    want = r.expected(rp)
    r.compare(want, "replay on other views")
    assert [w["status"] for w in want] == [0, ref.PRS_ERR_RANGE]


# ---- 9. the sphere and the chain -------------------------------------------------------------------------------------------------------
def test_the_sphere_scene_equals_the_restatement(hip_ctx):
    s = cases.SPHERE
    seq, origin = cases.sphere_scene()
    nx, ny, nz = s["dims"]
    volume = tsdf_ref.integrate(seq, tsdf_ref.params(s["camera"], voxel_size=s["voxel_size"], truncation=s["truncation"]), origin,
                                np.zeros((nz, ny, nx, 2), F))["volume"]
    poses = np.stack([seq["pose"][0], seq["pose"][1], cases.pose_about(s["centre"], 0.25, 2.0), cases.pose_about(s["centre"], -0.2, 1.6)])
    r = Rig(hip_ctx, [volume], [origin], [dict(pose=poses, n_views=4)], 4, s["rows"], s["cols"])
    want = r.check(*params_pair(ops, s["camera"], voxel_size=s["voxel_size"], step=s["voxel_size"]))[0]
    assert want["n_hit"].min() > 700 and normals_of(want).min() > 600


def test_integrate_raycast_and_the_dense_cloud_through_ops(hip_ctx):
    """the integrator's volume is read in place by the raycast, whose depth is read in place by the dense cloud; everything equals the
    restatements chained on the CPU"""
    import torch

    import depth_cloud_ref as dref
    B, frames, views, dims = 1, 3, 2, DIMS
    seq = tsdf_rig.scene((12,), dims, frames, "f32", bad=True)
    origin = tsdf_rig.origin_in_front(dims)
    fp, frp = tsdf_rig.params_pair(ops)
    fusedv = tsdf_ref.integrate(seq, frp, origin, np.zeros((dims[2], dims[1], dims[0], 2), F))
    looks = views_of((12,), views)
    p, rp = params_pair(ops)
    want = ref.raycast(looks, rp, origin, fusedv["volume"], views, ROWS, COLS)
    ckw = dict(range_min=0.1, range_max=10.0, scale=1.0)
    cloud = dref.depth_cloud(dict(depth=want["depth"], n_images=views, pose=looks["pose"]), dref.params(K, **ckw), views * ROWS * COLS)
    n = cloud["n_out"]
    assert n == want["n_hit"].sum() > 200

    dev = torch.device("cuda", 0)
    vb = ops.TsdfVolumeBatch(B, *dims, frames, ROWS, COLS)
    vb.origin.copy_(torch.from_numpy(origin[None]))
    vb.integrate(hip_ctx, fp, torch.from_numpy(seq["depth"]).to(dev).unsqueeze(0), torch.from_numpy(seq["pose"]).to(dev).unsqueeze(0))
    rb = ops.TsdfRaycastBatch(hip_ctx, vb, views, ROWS, COLS)
    t_looks = torch.from_numpy(looks["pose"]).to(dev).unsqueeze(0)
    depth, normal, n_hit = rb.run(p, t_looks)
    dc = ops.DepthCloudBatch(B, views, ROWS, COLS, views * ROWS * COLS)
    dc.run(hip_ctx, ops.depth_cloud_params(K, depth_type="f32", **ckw), depth, t_looks, torch.tensor([views], dtype=torch.int32, device=dev))
    hip_ctx.synchronize()
    assert depth.data_ptr() == rb.depth.data_ptr() and rb.status.cpu().tolist() == [0] and rb.n_skipped.cpu().tolist() == [0]
    assert vb.volume.cpu().numpy().tobytes() == fusedv["volume"][None].tobytes()
    assert depth.cpu().numpy().tobytes() == want["depth"][None].tobytes() and normal.cpu().numpy().tobytes() == want["normal"][None].tobytes()
    assert n_hit.cpu().tolist() == [want["n_hit"].tolist()]
    got = dc.cloud_of(0)
    assert (got["status"], got["n_out"], got["n_total"]) == (0, n, cloud["n_total"])
    assert got["xyz"].tobytes() == cloud["xyz"][:n].tobytes()
