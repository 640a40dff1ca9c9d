"""The TSDF mesh where byte offsets pass 2^32: two sequences of 1024 x 1024 x 513 voxels, 2^32 + 2^23 bytes each, so the second
sequence's volume begins past 2^32 bytes and its last layers lie past 2^33, as in tests/test_tsdf_limits_gpu.py.  The volumes are zero
(never observed) except for thin slabs planted directly, with no integrate call, in the first three and the last three layers of both
sequences: patches of tilted planes that differ between the four places, so an offset that lost its upper bits would read the other
sequence's slab or find none.

Of the workspace's three parts the two rows of chunk counts stay small (2 x 525312 int32 each); the rank map holds an int32 a voxel,
2^31 + 2^22 bytes a sequence, so the second sequence's map begins past 2^31 bytes and the ranks of its last slab lie past 2^32: that
is the workspace offset this case drives past 2^32.  The outputs are small.

The restatement runs on the slabs alone.  A slab of four layers whose innermost layer is empty is a faithful piece of the volume: no
cube reaches from it into the layers between.  For the last slab the restatement gets the origin moved up by nz - 4 layers, which is
exact in float32 here (the voxel size is a power of two and the origin a small multiple of it), and its cube and edge rows are moved
back by the voxels of the layers below, its ranks by the vertices of the first slab."""
import time

import numpy as np
import pytest

import big_batch as bb
import tsdf_mesh_ref as ref
import tsdf_ref
from tsdf_rig import K
from srrg2_proslam_amd import ops

pytestmark = pytest.mark.gpu
F = np.float32
GB = 1 << 30
DIMS = (1024, 1024, 513)
VS = 2.0 ** -6
LAYERS = 4           # of a slab handed to the restatement; the planted values fill three of them
NV, NQ = 4096, 4096


@pytest.fixture(autouse=True)
def report():
    """prints what the test took: seconds and the peak of device memory"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print("\n[tsdf mesh limits] %.1f s, peak %.2f GB of device memory" % (time.time() - t0, torch.cuda.max_memory_allocated() / 1e9))
    bb.release()


def patch(key, top):
    """a slab [LAYERS, ny, nx, 2] that is empty but for a 40 x 30 patch of a tilted plane in three layers: the lowest three, or with
    `top` the highest three.  i0, j0: where the patch begins"""
    nx, ny, _ = DIMS
    slab = np.zeros((LAYERS, ny, nx, 2), F)
    i0, j0 = 5 + 200 * key, 900 - 250 * key
    k, j, i = np.meshgrid(np.arange(3), np.arange(30), np.arange(40), indexing="ij")
    t = np.clip((0.02 + 0.01 * key) * (i - 20) + 0.03 * (j - 15) + 0.6 * (k - 1) + 0.11, -1, 1).astype(F)
    k0 = 1 if top else 0
    slab[k0:k0 + 3, j0:j0 + 30, i0:i0 + 40, 0] = t
    slab[k0:k0 + 3, j0:j0 + 30, i0:i0 + 40, 1] = 1
    return slab


def test_a_volume_and_a_rank_map_that_pass_4_gib(hip_ctx):
    import torch
    nx, ny, nz = DIMS
    voxels = nx * ny * nz
    assert voxels * 8 > 1 << 32 and voxels <= 0x7fffffff // 3 and 2 * voxels * 4 > 1 << 32
    bb.need_memory(16 * GB)  # the volumes hold 8.6 GB, the workspace 4.3 GB
    vb = ops.TsdfVolumeBatch(2, nx, ny, nz, 1, 2, 2)
    assert vb.volume[1].data_ptr() - vb.volume.data_ptr() == (1 << 32) + (1 << 23)
    origins = np.array([[-8.0, -8.0, 1.0, 0.0], [-8.0 + 3 * VS, -8.0, 1.0 + 5 * VS, 0.0]], F)
    vb.origin.copy_(torch.from_numpy(origins))
    slabs = {}
    for b in range(2):
        for top in (False, True):
            slab = slabs[b, top] = patch(2 * b + top, top)
            k0 = nz - LAYERS if top else 0
            vb.volume[b, k0:k0 + LAYERS].copy_(torch.from_numpy(slab))
    p = ops.tsdf_params(K, voxel_size=VS, truncation=4 * VS, min_weight=1.0)
    rp = tsdf_ref.params(K, voxel_size=VS, truncation=4 * VS, min_weight=1.0)
    mb = ops.TsdfMeshBatch(vb, NV, NQ)
    assert mb.workspace.numel() == 2 * 2 * 525312 * 4 + 2 * voxels * 4
    bb.fill_sentinel(mb.vertex, mb.normal, mb.quad, mb.cube, mb.edge)
    mb.run(hip_ctx, p)
    hip_ctx.synchronize()
    assert mb.status.cpu().tolist() == [0, 0]
    for b in range(2):
        rows = {k: [] for k in ("vertex", "normal", "quad", "cube", "edge")}
        n_v = n_q = 0
        for top in (False, True):
            below = (nz - LAYERS) * nx * ny if top else 0
            origin = origins[b].copy()
            if top:
                origin[2] = origin[2] + F(nz - LAYERS) * F(VS)
                assert float(origin[2]) == float(origins[b][2]) + (nz - LAYERS) * VS   # exact
            w = ref.mesh(slabs[b, top], rp, origin, NV, NQ)
            assert w["status"] == 0 and w["n_vertices"] > 500 and w["n_quads"] > 300, (b, top, w["n_vertices"], w["n_quads"])
            v, q = w["n_vertices"], w["n_quads"]
            rows["vertex"].append(w["vertex"][:v])
            rows["normal"].append(w["normal"][:v])
            rows["cube"].append((w["cube"][:v].astype(np.int64) + below).astype(np.int32))
            rows["edge"].append((w["edge"][:q].astype(np.int64) + 3 * below).astype(np.int32))
            rows["quad"].append(w["quad"][:q] + np.int32(n_v))
            n_v, n_q = n_v + v, n_q + q
        assert (int(mb.n_vertices[b]), int(mb.n_vertices_total[b]), int(mb.n_quads[b]), int(mb.n_quads_total[b])) == (n_v, n_v, n_q, n_q), b
        for name, n in (("vertex", n_v), ("normal", n_v), ("cube", n_v), ("quad", n_q), ("edge", n_q)):
            got = getattr(mb, name)[b].cpu().numpy()
            assert got[:n].tobytes() == np.concatenate(rows[name]).tobytes(), (b, name)
            assert (got[n:].view(np.uint8) == bb.SENTINEL).all(), (b, name, "behind the count")
        # the second sequence's last slab lies where a 32-bit byte offset into the volume and into the rank map has wrapped (the first
        # sequence's ends 2^23 bytes past 2^32, its last four layers begin just below)
        last = int(rows["cube"][1].max())
        assert ((b * voxels + last) * 8 > (1 << 32)) == (b == 1) and ((b * voxels + last) * 4 > (1 << 32)) == (b == 1)
    del mb, vb
