"""The TSDF raycast where byte offsets pass 2^32, in the volume it reads and in the normal image it writes.

1. one volume of 1024 x 1024 x 528 voxels, 2^32 + 2^27 bytes, empty but for a wall planted in its last eight layers, which lie past
   2^32 bytes; a 24 x 20 image looks at it through the empty layers.  An offset that lost its upper bits would read the first layers,
   which hold nothing, and hit nothing.  The restatement is evaluated on the planted slab alone.
2. one view of 16385 x 16384 pixels of a small volume: normal has 2^32 + 2^18 bytes, so the last row lies past 2^32.  The camera's
   centre lies on row 16380: the rows that hit anything are the last ones.  The first row, the last row and every row that hits are
   compared with the restatement, every other row holds zeros, and n_hit is the sum over the compared rows."""
import time

import numpy as np
import pytest

import big_batch as bb
import tsdf_raycast_ref as ref
from tsdf_raycast_rig import fused, params_pair
from tsdf_rig import COLS, ROWS, K
from srrg2_proslam_amd import ops

pytestmark = pytest.mark.gpu
F = np.float32
GB = 1 << 30
EYE = np.eye(4, dtype=F).reshape(1, 16)


@pytest.fixture(autouse=True)
def report():
    """prints what the test took: seconds and the peak of device memory"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print("\n[tsdf raycast limits] %.1f s, peak %.2f GB of device memory" % (time.time() - t0, torch.cuda.max_memory_allocated() / 1e9))
    bb.release()


def test_a_surface_in_the_layers_of_a_volume_past_4_gib(hip_ctx):
    import torch
    nx, ny, nz = 1024, 1024, 528
    vs, trunc, slab_layers = 0.01, 0.03, 8
    assert nx * ny * nz * 8 > 1 << 32 and nx * ny * nz <= 0x7fffffff // 3
    bb.need_memory(6 * GB)
    k0 = nz - slab_layers
    assert ((k0 * ny) * nx) * 8 > 1 << 32     # the whole slab lies past 2^32 bytes
    # a wall four layers from the volume's back, tilted a little, every voxel of the slab observed once
    zc = (1.0 + (np.arange(k0, nz) + 0.5) * vs)[:, None, None]
    tilt = np.linspace(-0.01, 0.01, nx)[None, None, :] + np.linspace(-0.005, 0.005, ny)[None, :, None]
    slab = np.zeros((slab_layers, ny, nx, 2), F)
    slab[..., 0] = np.clip(((1.0 + (nz - 4) * vs + tilt) - zc) / trunc, -1.0, 1.0)
    slab[..., 1] = 1.0
    origin = np.array([-nx * vs / 2 + 0.003, -ny * vs / 2, 1.0, 0.0], F)
    p, rp = params_pair(ops, voxel_size=vs, step=vs)
    want = ref.raycast(dict(pose=EYE), rp, origin, slab, 1, ROWS, COLS, slab=(k0, nz))
    assert want["n_hit"][0] > 400 and (want["normal"][..., 3] == 1).sum() > 400

    vb = ops.TsdfVolumeBatch(1, nx, ny, nz, 1, ROWS, COLS)
    vb.origin.copy_(torch.from_numpy(origin[None]))
    vb.volume[0, k0:].copy_(torch.from_numpy(slab))
    rb = ops.TsdfRaycastBatch(hip_ctx, vb, 1, ROWS, COLS)
    depth, normal, n_hit = rb.run(p, torch.from_numpy(EYE[None]).cuda())
    hip_ctx.synchronize()
    assert rb.status.cpu().tolist() == [0] and rb.n_skipped.cpu().tolist() == [0] and n_hit.cpu().tolist() == [want["n_hit"].tolist()]
    assert depth[0].cpu().numpy().tobytes() == want["depth"].tobytes()
    assert normal[0].cpu().numpy().tobytes() == want["normal"].tobytes()
    del vb, rb


def test_a_normal_image_past_4_gib(hip_ctx):
    import torch
    rows, cols = 16385, 16384
    assert rows * cols * 16 > 1 << 32 and (rows - 1) * cols * 16 == 1 << 32
    bb.need_memory(8 * GB)
    dims = (17, 12, 9)
    volume, origin = fused((3,) + dims, dims)
    camera = dict(K, cx=cols / 2 - 0.5, cy=16380.0)
    p, rp = params_pair(ops, camera)
    vb = ops.TsdfVolumeBatch(1, *dims, 1, 2, 2)
    vb.origin.copy_(torch.from_numpy(origin[None]))
    vb.volume.copy_(torch.from_numpy(volume[None].copy()))
    rb = ops.TsdfRaycastBatch(hip_ctx, vb, 1, rows, cols)
    bb.fill_sentinel(rb.depth, rb.normal, rb.n_hit)
    depth, normal, n_hit = rb.run(p, torch.from_numpy(EYE[None]).cuda())
    hip_ctx.synchronize()
    assert rb.status.cpu().tolist() == [0]
    hit_rows = torch.nonzero((depth[0, 0] != 0).any(dim=1)).reshape(-1).cpu().tolist()
    assert len(hit_rows) >= 10 and hit_rows[-1] == rows - 1 and hit_rows[0] > rows - 40   # the last row, past 2^32 bytes, hits
    compared = sorted(set([0, rows - 1] + hit_rows))
    v, u = np.meshgrid(np.array(compared), np.arange(cols), indexing="ij")
    want = ref.raycast(dict(pose=EYE), rp, origin, volume, 1, rows, cols, pixels=(v, u))
    assert want["n_hit"][0] > 100 and (want["depth"][0][-1] > 0).sum() > 5 and (want["normal"][0][-1, :, 3] == 1).sum() > 3
    index = torch.tensor(compared, device="cuda")
    assert depth[0, 0, index].cpu().numpy().tobytes() == want["depth"][0].tobytes()
    assert normal[0, 0, index].cpu().numpy().tobytes() == want["normal"][0].tobytes()
    assert n_hit.cpu().tolist() == [[int(want["n_hit"][0])]]
    rest = torch.ones(rows, dtype=torch.bool, device="cuda")
    rest[index] = False
    assert int(torch.count_nonzero(depth[0, 0].view(torch.int32)[rest])) == 0           # +0.0f everywhere else
    for chunk in torch.nonzero(rest).reshape(-1).split(2048):                               # 0.5 GB at a time
        assert int(torch.count_nonzero(normal[0, 0, chunk].view(torch.int32))) == 0
    del vb, rb
