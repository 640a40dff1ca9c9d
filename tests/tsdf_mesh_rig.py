"""What the TSDF mesh's tests share: the volumes of the cases, built on the host so that their conditions can be looked at without a
GPU (tests/test_tsdf_mesh_ref.py), and a Rig that owns the device arrays of prs_tsdf_mesh_batch_run for a batch of them, runs the
entry point on sentinel-filled outputs and compares every output, byte for byte, with tests/tsdf_mesh_ref.py: what the rule writes,
and the sentinel everywhere else -- the rows from the counts on, an output that was not asked for, and one sequence's worth of every
output behind the batch.  Test infrastructure only."""
import ctypes as C
import functools

import numpy as np

import tsdf_cases
import tsdf_mesh_ref as ref
import tsdf_ref
from tsdf_rig import SENTINEL, sentinel

F = np.float32
VS, TRUNC = 0.05, 0.15
ROWS = ("vertex", "normal", "quad", "cube", "edge")
COUNTS = ("n_vertices", "n_vertices_total", "n_quads", "n_quads_total", "status")
OPTIONAL = ("normal", "cube", "edge")
SPHERE_CENTRE, SPHERE_RADIUS = np.array([0.02, 0.01, 0.015]), 0.22


def host_params(min_weight=1.0, voxel_size=VS):
    """tsdf_ref.params of which the mesh reads voxel_size and min_weight"""
    return tsdf_ref.params(tsdf_cases.K, voxel_size=voxel_size, truncation=TRUNC, min_weight=min_weight)


def _frozen(volume, origin):
    volume.setflags(write=False)
    origin.setflags(write=False)
    return volume, origin


@functools.lru_cache(maxsize=None)
def sphere_volume():
    """(volume [15, 13, 14, 2], origin [4]): the analytic sphere of radius 0.22 about SPHERE_CENTRE, weight 1 everywhere.  Shared by
    the tests: do not write into it"""
    nx, ny, nz = 14, 13, 15
    origin = np.array([-0.33, -0.31, -0.36, 0.0])
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    c = origin[:3] + (np.stack([i, j, k], axis=-1) + 0.5) * VS
    t = np.clip((np.linalg.norm(c - SPHERE_CENTRE, axis=-1) - SPHERE_RADIUS) / TRUNC, -1, 1)
    return _frozen(np.stack([t, np.ones_like(t)], axis=-1).astype(F), origin.astype(F))


@functools.lru_cache(maxsize=None)
def plane_volume(dims):
    """(volume, origin): a tilted plane through the whole grid of dims = (nx, ny, nz) voxels, weight 1 everywhere"""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    t = np.clip((0.31 * (i - nx / 2) + 0.2 * (j - ny / 2) + 0.9 * (k + 0.5 - nz / 2) + 0.13) * VS / TRUNC, -1, 1)
    return _frozen(np.stack([t, np.ones_like(t)], axis=-1).astype(F), np.array([0.1, -0.2, 0.3, 0.0], F))


@functools.lru_cache(maxsize=None)
def fused_sphere():
    """(volume [27, 26, 28, 2], origin): tsdf_cases.sphere_scene() fused by the fusion's restatement"""
    s = tsdf_cases.SPHERE
    seq, origin = tsdf_cases.sphere_scene()
    p = tsdf_ref.params(s["camera"], voxel_size=s["voxel_size"], truncation=s["truncation"])
    nx, ny, nz = s["dims"]
    return _frozen(tsdf_ref.integrate(seq, p, origin, np.zeros((nz, ny, nx, 2), F))["volume"], np.array(origin, F))


@functools.lru_cache(maxsize=None)
def random_volume(dims=(28, 26, 27), seed=5):
    """(volume, origin): tsdf uniform in [-1.2, 1.2], weights 0, 1 and 2 (min_weight 1 leaves a third unobserved), and one voxel in
    fifty each NaN, +inf and -inf"""
    nx, ny, nz = dims
    rng = np.random.default_rng([91, seed])
    t = rng.uniform(-1.2, 1.2, (nz, ny, nx)).astype(F)
    r = rng.random(t.shape)
    t[r < 0.02] = np.nan
    t[(r >= 0.02) & (r < 0.04)] = np.inf
    t[(r >= 0.04) & (r < 0.06)] = -np.inf
    w = rng.integers(0, 3, t.shape).astype(F)
    return _frozen(np.stack([t, w], axis=-1), np.array([-0.7, -0.65, 1.3, 0.0], F))


def empty_volume(dims=(28, 26, 27)):
    nx, ny, nz = dims
    return np.zeros((nz, ny, nx, 2), F), np.array([0.0, 0.0, 0.0, 0.0], F)


@functools.lru_cache(maxsize=None)
def totals(maker, *args):
    """(n_vertices_total, n_quads_total) of a case at min_weight 1"""
    volume, origin = maker(*args)
    w = ref.mesh(volume, host_params(), origin, 0, 0, count_only=True)
    return w["n_vertices_total"], w["n_quads_total"]


class Rig:
    """the device side of B volumes of one size and the meshes taken out of them"""

    def __init__(self, ctx, volumes, origins, vertex_stride, quad_stride, take=None):
        import torch
        from srrg2_proslam_amd import _lib_tsdf_mesh
        self.ctx, self.lib, self.torch = ctx, _lib_tsdf_mesh.load(), torch
        self.B, self.vcap, self.qcap = len(volumes), int(vertex_stride), int(quad_stride)
        nz, ny, nx = volumes[0].shape[:3]
        self.dims = (nx, ny, nz)
        B, nv, nq = self.B, self.vcap, self.qcap
        self.extra = 1 if take is None else 0  # a sequence's worth of every output behind the batch: it keeps the sentinel
        E = B + self.extra
        z = (lambda shape, dt, align, name: torch.zeros(shape, dtype=dt, device="cuda")) if take is None else take
        i32, f32 = torch.int32, torch.float32
        self.t = dict(origin=z((B, 4), f32, 4, "origin"), volume=z((B, nz, ny, nx, 2), f32, 16, "volume"),
                      vertex=z((E, nv, 4), f32, 16, "vertex"), normal=z((E, nv, 4), f32, 16, "normal"), quad=z((E, nq, 4), i32, 16, "quad"),
                      cube=z((E, nv), i32, 4, "cube"), edge=z((E, nq), i32, 4, "edge"),
                      workspace=z((int(self.lib.prs_tsdf_mesh_workspace_bytes(B, nx, ny, nz)),), torch.uint8, 16, "workspace"))
        for name in COUNTS:
            self.t[name] = z((E,), i32, 4, name)
        self.upload(volumes, origins)

    def put(self, name, host):
        self.t[name].copy_(self.torch.from_numpy(np.ascontiguousarray(host)))

    def get(self, name):
        return self.t[name].cpu().numpy()

    def upload(self, volumes, origins):
        self.volumes = [np.asarray(v, F) for v in volumes]
        self.origins = np.stack([np.asarray(o, F) for o in origins])
        self.put("origin", self.origins)
        self.put("volume", np.stack(self.volumes))

    def fill_outputs(self):
        for name in ROWS + COUNTS:
            self.t[name].view(self.torch.uint8).fill_(SENTINEL)

    def descriptor(self, outputs=OPTIONAL, count_only=False, vertex_stride=None, quad_stride=None):
        from srrg2_proslam_amd import _lib_tsdf_mesh
        d = _lib_tsdf_mesh.TsdfMeshBatch()
        d.batch = self.B
        d.nx, d.ny, d.nz = self.dims
        d.vertex_stride = self.vcap if vertex_stride is None else vertex_stride
        d.quad_stride = self.qcap if quad_stride is None else quad_stride
        for name in ("origin", "volume", "workspace") + COUNTS:
            setattr(d, name, self.t[name].data_ptr())
        if not count_only:
            for name in ("vertex", "quad") + tuple(outputs):
                setattr(d, name, self.t[name].data_ptr())
        return d

    def run(self, p, **kw):
        return self.lib.prs_tsdf_mesh_batch_run(self.ctx._h, C.byref(p), C.byref(self.descriptor(**kw)))

    def expected(self, rp, outputs=OPTIONAL, count_only=False, vertex_stride=None, quad_stride=None):
        """the outputs of every sequence after a call on sentinel-filled arrays"""
        nv = self.vcap if vertex_stride is None else vertex_stride
        nq = self.qcap if quad_stride is None else quad_stride
        out = []
        for b in range(self.B):
            before = dict(vertex=sentinel((nv, 4), F), normal=sentinel((nv, 4), F), quad=sentinel((nq, 4), np.int32),
                          cube=sentinel((nv,), np.int32), edge=sentinel((nq,), np.int32))
            want = ref.mesh(self.volumes[b], rp, self.origins[b], nv, nq, before, count_only=count_only)
            for name in ROWS:
                if count_only or (name in OPTIONAL and name not in outputs):
                    want[name] = before[name]
            out.append(want)
        return out

    def compare(self, want, what=""):
        got = {k: self.get(k) for k in ROWS + COUNTS}
        for b, w in enumerate(want):
            assert [int(got[k][b]) for k in COUNTS] == [w[k] for k in COUNTS], (what, b, COUNTS)
        for name in ROWS:
            flat = got[name].reshape(-1)
            n = want[0][name].size  # the call sees [B][stride] rows at the head of the rig's arrays
            for b, w in enumerate(want):
                same = flat[b * n:(b + 1) * n].view(np.uint32) == w[name].reshape(-1).view(np.uint32)
                assert same.all(), (what, b, name, np.flatnonzero(~same)[:4].tolist())
            assert (flat[self.B * n:].view(np.uint8) == SENTINEL).all(), (what, name, "behind the last sequence")
        for name in COUNTS:
            assert (got[name][self.B:].view(np.uint8) == SENTINEL).all(), (what, name, "behind the last sequence")

    def check(self, p, rp, what="", **kw):
        """runs the call on sentinel-filled outputs and compares every output -> the expectations"""
        self.fill_outputs()
        assert self.run(p, **kw) == 0, what
        self.ctx.synchronize()
        want = self.expected(rp, **kw)
        self.compare(want, what)
        return want
