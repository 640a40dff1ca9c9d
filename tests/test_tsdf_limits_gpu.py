"""TSDF fusion where byte offsets into the volume pass 2^32: two sequences of 1024 x 1024 x 513 voxels, 2^32 + 2^23 bytes each, so
the second sequence's volume begins past 2^32 bytes and its last layers lie past 2^33.  One image a sequence.  An offset that lost
its upper bits would land in the other sequence's volume one layer off, and the two sequences see different depths from different
origins: slabs of both volumes -- the first layers, the last layers, and layers of the middle -- are compared with the restatement
evaluated on those slabs alone, and the number of voxels with a weight with n_updates.  The surface call runs on the same volumes with
a small out_stride: the rows it keeps are the first crossings in raster order, which lie in the first layers, and equal the
restatement's on that slab."""
import time

import numpy as np
import pytest

import big_batch as bb
import tsdf_ref as ref
from tsdf_rig import COLS, ROWS, K, params_pair
from srrg2_proslam_amd import ops

pytestmark = pytest.mark.gpu
F = np.float32
GB = 1 << 30
DIMS = (1024, 1024, 513)
VS, TRUNC = 0.01, 0.03
CAP = 1000


@pytest.fixture(autouse=True)
def report():
    """prints what the test took: seconds and the peak of device memory"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print("\n[tsdf limits] %.1f s, peak %.2f GB of device memory" % (time.time() - t0, torch.cuda.max_memory_allocated() / 1e9))
    bb.release()


def test_a_volume_that_begins_past_4_gib(hip_ctx):
    import torch
    nx, ny, nz = DIMS
    assert nx * ny * nz * 8 > 1 << 32 and nx * ny * nz <= 0x7fffffff // 3
    bb.need_memory(16 * GB)  # the volumes hold 8.6 GB; counting the weights takes as much again for a moment
    # the left half of the image sees a wall in the first layers, the right half one in the last layers
    seqs, origins = [], []
    for b in range(2):
        depth = np.empty((1, ROWS, COLS), F)
        depth[:, :, :COLS // 2] = 1.02 + 0.004 * b
        depth[:, :, COLS // 2:] = 1.0 + (nz - 1.2) * VS - 0.004 * b
        depth += np.linspace(0, 0.01, ROWS, dtype=F)[None, :, None]
        seqs.append(dict(depth=depth, pose=np.eye(4, dtype=F).reshape(1, 16), n_images=1))
        origins.append(np.array([-nx * VS / 2 + 0.003 * b, -ny * VS / 2, 1.0, 0.0], F))
    p, rp = params_pair(ops, voxel_size=VS, truncation=TRUNC)
    vb = ops.TsdfVolumeBatch(2, nx, ny, nz, 1, ROWS, COLS, out_stride=CAP)
    assert vb.volume[1].data_ptr() - vb.volume.data_ptr() == (1 << 32) + (1 << 23)
    vb.origin.copy_(torch.from_numpy(np.stack(origins)))
    t_depth = torch.from_numpy(np.stack([s["depth"] for s in seqs])).cuda()
    t_pose = torch.from_numpy(np.stack([s["pose"] for s in seqs])).cuda()
    vb.integrate(hip_ctx, p, t_depth, t_pose)
    xyz, normal, n_out = vb.surface(hip_ctx, p)
    hip_ctx.synchronize()
    assert vb.status.cpu().tolist() == [0, 0] and vb.n_skipped.cpu().tolist() == [0, 0]
    for b in range(2):
        seen = 0
        for k0, k1 in ((0, 6), (255, 257), (nz - 4, nz)):
            want = ref.integrate(seqs[b], rp, origins[b], np.zeros((k1 - k0, ny, nx, 2), F), slab=(k0, k1))
            got = vb.volume[b, k0:k1].cpu().numpy()
            same = got.view(np.uint32) == want["volume"].view(np.uint32)
            assert same.all(), (b, k0, np.argwhere(~same)[:4].tolist())
            assert want["n_updates"][0] > 1000, (b, k0)  # the slab holds voxels the image updated
            seen += int(want["n_updates"][0])
        weighted = int((vb.volume[b, ..., 1] > 0).sum().item())
        assert weighted == int(vb.n_updates[b, 0].item()) > seen  # one image into an empty volume: a weight is an update
        # the first CAP crossings lie in the first layers
        slab = vb.volume[b, :8].cpu().numpy()
        want = ref.surface(slab, rp, origins[b], CAP)
        assert want["n_total"] > CAP and (want["cell"] // 3 // (nx * ny)).max() < 5  # none of them on the slab's last layers
        assert int(vb.surface_status[b].item()) == ref.PRS_ERR_CAPACITY and int(n_out[b].item()) == CAP
        assert int(vb.n_total[b].item()) > want["n_total"]  # the far wall's crossings are counted too
        assert xyz[b].cpu().numpy().tobytes() == want["xyz"].tobytes()
        assert normal[b].cpu().numpy().tobytes() == want["normal"].tobytes()
        assert vb.cell[b].cpu().numpy().tobytes() == want["cell"].tobytes()
    del vb
