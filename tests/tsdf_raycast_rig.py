"""What the TSDF raycast's device tests share: the volumes of the tests, fused on the host by tests/tsdf_ref.py from the scenes of
tests/tsdf_rig.py, and a Rig that owns the device arrays of prs_tsdf_raycast_batch_run for a batch of them, runs the entry point on
sentinel-filled outputs and compares every output, byte for byte, with tests/tsdf_raycast_ref.py: what the rule writes, and the
sentinel everywhere else -- the pitch padding, the views from n_views on, a refused sequence, and one sequence's worth of every output
behind the batch.  Test infrastructure only."""
import ctypes as C
import functools

import numpy as np

import tsdf_raycast_ref as ref
import tsdf_ref
import tsdf_rig
from tsdf_rig import COLS, ROWS, SENTINEL, VS, K, sentinel

F = np.float32
OUTPUTS = ("depth", "normal", "n_hit", "n_skipped", "status")


@functools.lru_cache(maxsize=None)
def fused(key, dims, frames=3, weights=False):
    """(volume [nz, ny, nx, 2], origin [4]) of tsdf_rig.scene(key, dims, frames) fused by the fusion's restatement: the surface runs
    through the volume's middle.  weights: the images differ in where they hold depths, so the weights are 1, 2 and 3 mixed.  Shared by
    the tests: do not write into it"""
    seq = tsdf_rig.scene(key, dims, frames, "f32", bad=weights)
    origin = tsdf_rig.origin_in_front(dims)
    p = tsdf_ref.params(K, voxel_size=VS, truncation=tsdf_rig.TRUNC)
    volume = tsdf_ref.integrate(seq, p, origin, np.zeros((dims[2], dims[1], dims[0], 2), F))["volume"]
    volume.setflags(write=False)
    return volume, origin


def views_of(key, views, pose_stride=None, index=False, n_views=None, spread=0.05, yaw=0.1):
    """one sequence's poses near the world's origin that look down +z, as the raycast reads them"""
    rng = tsdf_rig.rng_of(9, *key)
    ps = pose_stride or views
    seq = dict(pose=tsdf_rig.look_down_z(rng, ps, spread, yaw), n_views=views if n_views is None else n_views)
    if index:
        seq["view_index"] = rng.permutation(ps)[:views].astype(np.int32)
    return seq


def params_pair(ops, camera=K, **kw):
    """(ops.tsdf_raycast_params, tsdf_raycast_ref.params) of the same settings"""
    kw = dict(dict(voxel_size=VS, step=VS, min_weight=1.0, range_min=0.1, range_max=10.0), **kw)
    return ops.tsdf_raycast_params(camera, **kw), ref.params(camera, **kw)


class Rig:
    """the device side of B volumes and the views rendered out of them"""

    def __init__(self, ctx, volumes, origins, seqs, views, rows=ROWS, cols=COLS, pad=0, take=None):
        import torch
        from srrg2_proslam_amd import _lib_tsdf_raycast
        self.ctx, self.lib, self.torch = ctx, _lib_tsdf_raycast.load(), torch
        self.B, self.views, self.rows, self.cols, self.pad = len(volumes), int(views), int(rows), int(cols), int(pad)
        nz, ny, nx = volumes[0].shape[:3]
        self.dims = (nx, ny, nz)
        self.ps = seqs[0]["pose"].shape[0]
        B, V = self.B, self.views
        self.extra = 1 if take is None else 0  # a sequence's worth of every output behind the batch: it keeps the sentinel
        E = B + self.extra
        z = (lambda shape, dt, align, name: torch.zeros(shape, dtype=dt, device="cuda")) if take is None else take
        i32, f32 = torch.int32, torch.float32
        self.t = dict(origin=z((B, 4), f32, 4, "origin"), volume=z((B, nz, ny, nx, 2), f32, 16, "volume"),
                      pose=z((B, self.ps, 16), f32, 4, "pose"), view_index=z((B, V), i32, 4, "view_index"),
                      n_views=z((B,), i32, 4, "n_views"), depth=z((E, V, self.rows, self.cols + pad), f32, 4, "depth"),
                      normal=z((E, V, self.rows, self.cols, 4), f32, 16, "normal"), n_hit=z((E, V), i32, 4, "n_hit"),
                      n_skipped=z((E,), i32, 4, "n_skipped"), status=z((E,), i32, 4, "status"),
                      workspace=z((int(self.lib.prs_tsdf_raycast_workspace_bytes(B, V)),), torch.uint8, 16, "workspace"))
        self.volumes = [np.asarray(v, F) for v in volumes]
        self.origins = np.stack([np.asarray(o, F) for o in origins])
        self.put("origin", self.origins)
        self.put("volume", np.stack(self.volumes))
        self.upload(seqs)

    def put(self, name, host):
        self.t[name].copy_(self.torch.from_numpy(np.ascontiguousarray(host)))

    def get(self, name):
        return self.t[name].cpu().numpy()

    def upload(self, seqs):
        self.seqs = seqs
        self.with_index = seqs[0].get("view_index") is not None
        self.put("n_views", np.array([s["n_views"] for s in seqs], np.int32))
        self.put("pose", np.stack([s["pose"] for s in seqs]))
        if self.with_index:
            self.put("view_index", np.stack([s["view_index"] for s in seqs]))

    def fill_outputs(self, names=OUTPUTS):
        """the sentinel into every byte of the outputs the caller owns: depth ends with the last pixel of its last row"""
        for name in names:
            t = self.t[name].reshape(-1)
            t[:t.numel() - (self.pad if name == "depth" and not self.extra else 0)].view(self.torch.uint8).fill_(SENTINEL)

    def descriptor(self, normal=True, n_hit=True, n_views=True, view_index=None):
        from srrg2_proslam_amd import _lib_tsdf_raycast
        d = _lib_tsdf_raycast.TsdfRaycastBatch()
        d.batch, d.views, d.rows, d.cols = self.B, self.views, self.rows, self.cols
        d.pitch, d.pose_stride = (self.cols + self.pad) * 4, self.ps
        d.nx, d.ny, d.nz = self.dims
        for name in ("origin", "volume", "pose", "depth", "n_skipped", "status", "workspace"):
            setattr(d, name, self.t[name].data_ptr())
        d.normal = self.t["normal"].data_ptr() if normal else None
        d.n_hit = self.t["n_hit"].data_ptr() if n_hit else None
        d.n_views = self.t["n_views"].data_ptr() if n_views else None
        d.view_index = self.t["view_index"].data_ptr() if (self.with_index if view_index is None else view_index) else None
        return d

    def run(self, p, **kw):
        return self.lib.prs_tsdf_raycast_batch_run(self.ctx._h, C.byref(p), C.byref(self.descriptor(**kw)))

    def expected(self, rp, normal=True, n_hit=True, n_views=True, view_index=None):
        """the outputs of every sequence after a call on sentinel-filled arrays"""
        V, rows, cols = self.views, self.rows, self.cols
        use_index = self.with_index if view_index is None else view_index
        out = []
        for b, s in enumerate(self.seqs):
            seq = dict(pose=s["pose"], view_index=s.get("view_index") if use_index else None, n_views=s["n_views"] if n_views else None)
            before = dict(depth=sentinel((V, rows, cols), F), normal=sentinel((V, rows, cols, 4), F), n_hit=sentinel((V,), np.int32))
            want = ref.raycast(seq, rp, self.origins[b], self.volumes[b], V, rows, cols, before)
            if not normal:
                want["normal"] = before["normal"]
            if not n_hit:
                want["n_hit"] = before["n_hit"]
            out.append(want)
        return out

    def compare(self, want, what=""):
        got = {k: self.get(k) for k in OUTPUTS}
        B = self.B
        for b, w in enumerate(want):
            assert int(got["status"][b]) == w["status"], (what, b, "status")
            assert int(got["n_skipped"][b]) == w["n_skipped"], (what, b, "n_skipped")
            assert got["n_hit"][b].tolist() == w["n_hit"].tolist(), (what, b, "n_hit")
            same = got["depth"][b][..., :self.cols].view(np.uint32) == w["depth"].view(np.uint32)
            assert same.all(), (what, b, "depth", np.argwhere(~same)[:4].tolist())
            same = got["normal"][b].view(np.uint32) == w["normal"].view(np.uint32)
            assert same.all(), (what, b, "normal", np.argwhere(~same)[:4].tolist())
        padding = got["depth"][:B][..., self.cols:].reshape(-1)
        padding = padding[:padding.size - (0 if self.extra else self.pad)]  # the last row's padding is not the caller's
        assert (np.frombuffer(padding.tobytes(), np.uint8) == SENTINEL).all(), (what, "the pitch padding")
        for name in OUTPUTS:
            assert (got[name][B:].view(np.uint8) == SENTINEL).all(), (what, name, "behind the last sequence")

    def check(self, p, rp, what="", **kw):
        """runs the call on sentinel-filled outputs and compares every output -> the expectations"""
        self.fill_outputs()
        assert self.run(p, **kw) == 0, what
        self.ctx.synchronize()
        want = self.expected(rp, **kw)
        self.compare(want, what)
        return want


def normals_of(w):
    """normals present per view of one sequence's expectation"""
    return (w["normal"][..., 3] == 1).reshape(w["normal"].shape[0], -1).sum(1)
