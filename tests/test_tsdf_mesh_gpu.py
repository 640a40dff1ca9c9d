"""prs_tsdf_mesh_batch_run on the device against tests/tsdf_mesh_ref.py, byte for byte: vertex, normal, quad, cube, edge, the four
counts and the status, and the sentinel wherever the rule writes nothing.

1. the tilted plane at sizes with no cube, one cube, and chunks that end inside a row of cubes
2. a batch of three volumes (the fused sphere, an empty volume, a random one with NaN and inf) in two orders
3. min_weight above every weight
4. the two strides exactly full and one short; a batch of which one sequence overflows
5. the count-only call; every subset of the optional outputs
6. refusals at the call and in the Python layer
7. a captured graph of integrate + mesh, replayed on other depth
8. the chain from the integrator through the mesh to a PLY file with faces"""
import ctypes as C
import itertools

import numpy as np
import pytest

import tsdf_mesh_ref as ref
import tsdf_mesh_rig as rig_
import tsdf_ref
import tsdf_rig
from tsdf_mesh_rig import COUNTS, OPTIONAL, ROWS, Rig, host_params
from tsdf_rig import SENTINEL, K
from srrg2_proslam_amd import _lib_tsdf_mesh, formats, ops

pytestmark = pytest.mark.gpu
F = np.float32
BIG = (28, 26, 27)   # the fused sphere's grid: 20 chunks


def device_params(min_weight=1.0, voxel_size=rig_.VS):
    return ops.tsdf_params(K, voxel_size=voxel_size, truncation=rig_.TRUNC, min_weight=min_weight)


P, RP = device_params(), host_params()


def trio(order=(0, 1, 2)):
    made = [rig_.fused_sphere(), rig_.empty_volume(BIG), rig_.random_volume(BIG)]
    return [made[i][0] for i in order], [made[i][1] for i in order]


# ---- 1. the plane ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(1, 5, 5), (2, 2, 2), (33, 5, 9), (70, 9, 6)], ids=lambda d: "%dx%dx%d" % d)
def test_the_tilted_plane(hip_ctx, dims):
    volume, origin = rig_.plane_volume(dims)
    nv, nq = rig_.totals(rig_.plane_volume, dims)
    r = Rig(hip_ctx, [volume, volume], [origin, origin + F(0.25)], nv + 2, nq + 3)
    want = r.check(P, RP, "plane")
    assert [(w["status"], w["n_vertices"], w["n_quads"]) for w in want] == [(0, nv, nq)] * 2
    if dims == (70, 9, 6):
        assert (nv, nq) == (184, 153)
        # four chunks, three of which hold cubes: a cube takes corners from two of them (a layer is 630 voxels), and a quad takes
        # ranks from cubes behind another chunk's base
        quad, cube = want[0]["quad"][:nq], want[0]["cube"][:nv]
        chunk_of_vertex = cube // 1024
        assert set(chunk_of_vertex.tolist()) == {0, 1, 2} and (np.ptp(chunk_of_vertex[quad], axis=1) > 0).any()
        assert ((cube + 630 + 70 + 1) // 1024 > chunk_of_vertex).any()
    if dims[0] == 1:
        assert len(ref.crossings(volume, RP, origin)[0]) > 0 and (nv, nq) == (0, 0)


# ---- 2. a batch of three ---------------------------------------------------------------------------------------------------------------
def test_a_batch_of_three_in_two_orders(hip_ctx):
    got = []
    for order in ((0, 1, 2), (2, 1, 0)):
        volumes, origins = trio(order)
        r = Rig(hip_ctx, volumes, origins, 13000, 6700)
        want = r.check(P, RP, "order %s" % (order,))
        totals = {i: (w["status"], w["n_vertices"], w["n_quads"]) for i, w in zip(order, want)}
        assert totals[0] == (0, 1007, 898) and totals[1] == (0, 0, 0) and totals[2][0] == 0 and totals[2][1] > 10000 and totals[2][2] > 6000
        got.append({i: {k: r.get(k)[b].tobytes() for k in ROWS + COUNTS} for b, i in enumerate(order)})
    assert got[0] == got[1]   # a sequence's bytes do not depend on its place in the batch
    undirected, _ = ref.edge_use(want[0]["quad"][:want[0]["n_quads"]])   # the random volume, first in the second order
    assert 4 in set(undirected.values())


# ---- 3. min_weight ---------------------------------------------------------------------------------------------------------------------
def test_min_weight_above_every_weight_and_at_the_largest(hip_ctx):
    volume, origin = rig_.random_volume((9, 8, 7), 3)
    r = Rig(hip_ctx, [volume], [origin], 400, 200)
    assert [(w["n_vertices"], w["n_quads"]) for w in r.check(device_params(3.0), host_params(3.0), "above")] == [(0, 0)]
    some = r.check(device_params(2.0), host_params(2.0), "at 2")[0]
    all_ = r.check(P, RP, "at 1")[0]
    assert 0 < some["n_vertices"] < all_["n_vertices"] and 0 < some["n_quads"] < all_["n_quads"]


# ---- 4. capacity -----------------------------------------------------------------------------------------------------------------------
def test_each_stride_exactly_full_and_one_short(hip_ctx):
    dims = (70, 9, 6)
    volume, origin = rig_.plane_volume(dims)
    nv, nq = rig_.totals(rig_.plane_volume, dims)
    r = Rig(hip_ctx, [volume, volume], [origin, origin], nv + 1, nq + 1)
    for vcap, qcap in ((nv, nq), (nv - 1, nq), (nv, nq - 1), (1, 1), (nv - 1, 1)):
        want = r.check(P, RP, "strides %d %d" % (vcap, qcap), vertex_stride=vcap, quad_stride=qcap)
        over = vcap < nv or qcap < nq
        assert all(w["status"] == (tsdf_ref.PRS_ERR_CAPACITY if over else 0) for w in want)
        assert all((w["n_vertices"], w["n_vertices_total"], w["n_quads"], w["n_quads_total"]) == (min(nv, vcap), nv, min(nq, qcap), nq) for w in want)
    # a quad behind a short vertex_stride names a rank that has no row
    short = r.expected(RP, vertex_stride=nv - 1, quad_stride=nq)[0]
    assert short["quad"][:nq].max() == nv - 1


def test_a_batch_of_which_one_sequence_overflows(hip_ctx):
    volumes, origins = trio()
    r = Rig(hip_ctx, volumes, origins, 1100, 1000)
    want = r.check(P, RP, "one overflows")
    assert [w["status"] for w in want] == [0, 0, tsdf_ref.PRS_ERR_CAPACITY]
    assert (want[2]["n_vertices"], want[2]["n_quads"]) == (1100, 1000) and want[2]["quad"].max() >= 1100


# ---- 5. count only, optional outputs -----------------------------------------------------------------------------------------------------
def test_count_only(hip_ctx):
    volumes, origins = trio()
    r = Rig(hip_ctx, volumes, origins, 8, 8)
    want = r.check(P, RP, "count only", count_only=True)
    assert [(w["status"], w["n_vertices"], w["n_quads"], w["n_vertices_total"], w["n_quads_total"]) for w in want[:2]] == \
        [(0, 0, 0, 1007, 898), (0, 0, 0, 0, 0)]
    assert want[2]["n_vertices_total"] > 10000
    for name in ROWS:
        assert (r.get(name).view(np.uint8) == SENTINEL).all(), name


@pytest.mark.parametrize("outputs", [s for n in range(4) for s in itertools.combinations(OPTIONAL, n)], ids=lambda s: "+".join(s) or "none")
def test_each_subset_of_the_optional_outputs(hip_ctx, outputs):
    dims = (9, 7, 6)
    volume, origin = rig_.plane_volume(dims)
    other, _ = rig_.random_volume(dims, 4)
    r = Rig(hip_ctx, [volume, other], [origin, origin], 200, 150)
    want = r.check(P, RP, "outputs %s" % (outputs,), outputs=outputs)
    assert (want[0]["n_vertices"], want[0]["n_quads"]) == (75, 58) and want[1]["n_quads"] > 0
    for name in OPTIONAL:
        assert (r.get(name).view(np.uint8) == SENTINEL).all() == (name not in outputs), name


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_call_level_refusals_write_nothing(hip_ctx):
    volume, origin = rig_.plane_volume((9, 7, 6))
    r = Rig(hip_ctx, [volume, volume], [origin, origin], 100, 100)
    lib, ctx = _lib_tsdf_mesh.load(), r.ctx._h
    r.fill_outputs()

    def run(d, q=P):
        return lib.prs_tsdf_mesh_batch_run(ctx, C.byref(q) if q is not None else None, C.byref(d) if d is not None else None)

    D = r.descriptor
    nan, inf = float("nan"), float("inf")
    # PRS_ERR_NULL
    assert run(None) == -1 and run(D(), None) == -1
    for field in ("origin", "volume", "workspace", "vertex", "quad") + COUNTS:   # vertex or quad alone: only one of the two is set
        d = D()
        setattr(d, field, None)
        assert run(d) == -1, field
    for field in OPTIONAL:                      # an optional output with the count-only call
        d = D(count_only=True)
        setattr(d, field, r.t[field].data_ptr())
        assert run(d) == -1, field
    # PRS_ERR_RANGE
    for field, value in (("batch", 0), ("nx", 0), ("ny", -3), ("nz", 0), ("vertex_stride", 0), ("quad_stride", -1)):
        d = D()
        setattr(d, field, value)
        assert run(d) == tsdf_ref.PRS_ERR_RANGE, (field, value)
    for field, value in (("voxel_size", 0.0), ("voxel_size", -0.05), ("voxel_size", nan), ("voxel_size", inf), ("min_weight", nan),
                         ("min_weight", -inf)):
        q = device_params()
        setattr(q, field, value)
        assert run(D(), q) == tsdf_ref.PRS_ERR_RANGE, (field, value)
    # PRS_ERR_UNSUPPORTED
    for field, step in (("volume", 8), ("vertex", 8), ("vertex", 4), ("normal", 8), ("quad", 8), ("quad", 4), ("workspace", 8), ("origin", 2),
                        ("cube", 2), ("edge", 1), ("n_vertices", 2), ("n_vertices_total", 2), ("n_quads", 2), ("n_quads_total", 1),
                        ("status", 2)):
        d = D()
        setattr(d, field, getattr(d, field) + step)
        assert run(d) == -5, field
    for nx, ny, nz in ((1024, 1024, 683), (1 << 16, 1 << 16, 1 << 16), (1 << 30, 1, 1)):
        d = D()
        d.nx, d.ny, d.nz = nx, ny, nz
        assert run(d) == -5, (nx, ny, nz)
    d = D()
    d.batch, d.nx, d.ny, d.nz = 1 << 14, 32, 32, 1024    # 2^24 chunks: more workgroups than one launch holds
    assert run(d) == -5
    r.ctx.synchronize()
    for name in ROWS + COUNTS:
        assert (r.get(name).view(np.uint8) == SENTINEL).all(), name
    assert b"prs_tsdf_mesh_batch_run" in lib.prs_last_error(ctx)
    # what the count-only call does not look at: the strides
    d = D(count_only=True)
    d.vertex_stride, d.quad_stride = 0, -7
    assert run(d) == 0 and run(D()) == 0
    r.ctx.synchronize()
    r.compare(r.expected(RP), "after the refusals")


def test_the_python_layer_refuses_what_the_library_refuses(hip_ctx):
    vb = ops.TsdfVolumeBatch(2, 5, 4, 3, 2, 5, 6)
    mb = ops.TsdfMeshBatch(vb, 7, 9, outputs=("cube",))
    assert tuple(mb.vertex.shape) == (2, 7, 4) and tuple(mb.quad.shape) == (2, 9, 4) and tuple(mb.cube.shape) == (2, 7)
    assert mb.normal is None and mb.edge is None
    d = mb.descriptor()
    assert (d.batch, d.nx, d.ny, d.nz, d.vertex_stride, d.quad_stride) == (2, 5, 4, 3, 7, 9)
    assert (d.volume, d.origin, d.vertex, d.quad, d.cube) == (vb.volume.data_ptr(), vb.origin.data_ptr(), mb.vertex.data_ptr(),
                                                              mb.quad.data_ptr(), mb.cube.data_ptr())
    assert d.normal is None and d.edge is None and d.workspace == mb.workspace.data_ptr()
    d = mb.descriptor(count_only=True)
    assert d.vertex is None and d.quad is None and d.cube is None and d.n_quads_total == mb.n_quads_total.data_ptr()
    for bad in (dict(vertex_stride=0), dict(quad_stride=-1), dict(outputs=("normal", "colour"))):
        with pytest.raises(ValueError):
            ops.TsdfMeshBatch(vb, **dict(dict(vertex_stride=4, quad_stride=4), **bad))
    for field, value in (("voxel_size", 0.0), ("voxel_size", float("nan")), ("min_weight", float("inf"))):
        q = device_params()
        setattr(q, field, value)
        with pytest.raises(ValueError):
            mb.run(hip_ctx, q)
        with pytest.raises(ValueError):
            mb.count(hip_ctx, q)
    with pytest.raises(ValueError):
        mb.mesh_of(2)


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------------
def test_a_captured_graph_of_integrate_and_mesh_replayed_on_other_depth(hip_ctx):
    import torch
    ctx = hip_ctx
    B, frames, dims = 2, 2, (17, 12, 9)
    fp, frp = tsdf_rig.params_pair(ops)
    origins = [tsdf_rig.origin_in_front(dims), tsdf_rig.origin_in_front(dims, shift=(0.02, -0.01))]
    dev = torch.device("cuda", 0)
    vb = ops.TsdfVolumeBatch(B, *dims, frames, tsdf_rig.ROWS, tsdf_rig.COLS)
    vb.origin.copy_(torch.from_numpy(np.stack(origins)))
    mb = ops.TsdfMeshBatch(vb, 400, 300)
    depth = torch.zeros((B, frames, tsdf_rig.ROWS, tsdf_rig.COLS), dtype=torch.float32, device=dev)
    pose = torch.zeros((B, frames, 16), dtype=torch.float32, device=dev)
    outputs = ("vertex", "normal", "quad", "cube", "edge") + COUNTS

    def load(key):
        seqs = [tsdf_rig.scene((key, b), dims, frames, "f32", bad=False) for b in range(B)]
        depth.copy_(torch.from_numpy(np.stack([s["depth"] for s in seqs])))
        pose.copy_(torch.from_numpy(np.stack([s["pose"] for s in seqs])))
        return seqs

    def enqueue():
        vb.clear()
        vb.integrate(ctx, fp, depth, pose)
        mb.run(ctx, fp)

    def expect(seqs, what):
        for b, s in enumerate(seqs):
            volume = tsdf_ref.integrate(s, frp, origins[b], np.zeros((dims[2], dims[1], dims[0], 2), F))["volume"]
            before = {k: sentinel_like(getattr(mb, k)[b]) for k in ROWS}
            w = ref.mesh(volume, frp, origins[b], 400, 300, before)
            assert w["status"] == 0 and w["n_quads"] > 50, (what, b)
            for k in outputs:
                got = getattr(mb, k)[b].cpu().numpy()
                assert got.tobytes() == np.asarray(w[k], got.dtype).tobytes(), (what, b, k)

    def sentinel_like(t):
        return tsdf_rig.sentinel(tuple(t.shape), np.float32 if t.dtype == torch.float32 else np.int32)

    def fill():
        for k in outputs:
            getattr(mb, k).view(torch.uint8).fill_(SENTINEL)

    first = load(21)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        enqueue()  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            enqueue()
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    torch.cuda.synchronize()
    for replay, key in enumerate((21, 22, 23)):
        seqs = first if replay == 0 else load(key)
        fill()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        expect(seqs, "replay %d" % replay)


# ---- 8. the chain ----------------------------------------------------------------------------------------------------------------------
def test_integrate_mesh_and_a_ply_with_faces_through_ops(hip_ctx, tmp_path):
    import torch
    import tsdf_cases
    s = tsdf_cases.SPHERE
    seq, origin = tsdf_cases.sphere_scene()
    nx, ny, nz = s["dims"]
    fp = ops.tsdf_params(s["camera"], voxel_size=s["voxel_size"], truncation=s["truncation"], depth_type="f32")
    dev = torch.device("cuda", 0)
    vb = ops.TsdfVolumeBatch(1, nx, ny, nz, len(seq["pose"]), s["rows"], s["cols"])
    vb.origin.copy_(torch.from_numpy(origin[None]))
    vb.integrate(hip_ctx, fp, torch.from_numpy(seq["depth"]).to(dev).unsqueeze(0), torch.from_numpy(seq["pose"]).to(dev).unsqueeze(0))
    mb = ops.TsdfMeshBatch(vb, 1100, 900)
    nvt, nqt = mb.count(hip_ctx, fp)
    hip_ctx.synchronize()
    assert (nvt.cpu().tolist(), nqt.cpu().tolist(), mb.n_vertices.cpu().tolist(), mb.status.cpu().tolist()) == ([1007], [898], [0], [0])
    vertex, quad, n_vertices, n_quads = mb.run(hip_ctx, fp)
    hip_ctx.synchronize()
    volume, _ = rig_.fused_sphere()
    assert vb.volume.cpu().numpy().tobytes() == volume[None].tobytes()
    want = ref.mesh(volume, host_params(), origin, 1100, 900)
    assert (n_vertices.cpu().tolist(), n_quads.cpu().tolist()) == ([1007], [898])
    xyz, normal, triangles = mb.mesh_of(0)
    assert xyz.is_cuda and triangles.dtype == torch.int32 and tuple(triangles.shape) == (2 * 898, 3)
    assert xyz.cpu().numpy().tobytes() == want["vertex"][:1007].tobytes() and normal.cpu().numpy().tobytes() == want["normal"][:1007].tobytes()
    assert triangles.cpu().numpy().tolist() == ref.triangles(want["quad"][:898]).tolist()
    path = str(tmp_path / "sphere.ply")
    formats.write_ply(path, xyz.cpu().numpy(), normals=normal.cpu().numpy(), faces=triangles.cpu().numpy())
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + 11
    header = raw[:end].decode("ascii").splitlines()
    assert "element vertex 1007" in header and "element face 1796" in header and "property list uchar int vertex_indices" in header
    body = raw[end:]
    vertices = np.frombuffer(body[:1007 * 24], "<f4").reshape(1007, 6)
    assert vertices.tobytes() == np.concatenate([want["vertex"][:1007, :3], want["normal"][:1007, :3]], axis=1).tobytes()
    faces = np.frombuffer(body[1007 * 24:], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert len(faces) == 1796 and (faces["n"] == 3).all() and faces["v"].tolist() == ref.triangles(want["quad"][:898]).tolist()
    # a sequence that overflowed has no mesh to hand out
    small = ops.TsdfMeshBatch(vb, 1006, 900)
    small.run(hip_ctx, fp)
    hip_ctx.synchronize()
    with pytest.raises(ValueError):
        small.mesh_of(0)
