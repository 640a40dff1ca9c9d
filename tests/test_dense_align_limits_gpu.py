"""The dense aligner where byte offsets pass 2^32: one pair of 16385 x 16384 pixels, whose model_normal has 2^32 + 2^18 bytes, at
step 64, so that only 257 x 256 samples are computed.  The last row of samples is the image's last row, which lies past 2^32 bytes in
model_normal; the estimate moves points along x and turns them about y only and the camera's centre lies near that row, so those
samples meet the model in that very row.  The model is a constant plane filled on the device.  Its normals are one of three by bands
of 64 rows (a plane with one normal holds three degrees only) and a fourth in the last row: an offset that lost its upper bits would
read another normal.  The live rows repeat one pattern.  The restatement is fed np.broadcast_to views and a look-up by row: the host
holds no array of the images' size."""
import time

import numpy as np
import pytest

import big_batch as bb
import dense_align_cases as cases
import dense_align_ref as ref
import dense_align_rig as rig_
from srrg2_proslam_amd import ops

pytestmark = pytest.mark.gpu
F = np.float32
GB = 1 << 30


@pytest.fixture(autouse=True)
def report():
    """prints what the test took: seconds and the peak of device memory"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print("\n[dense align limits] %.1f s, peak %.2f GB of device memory" % (time.time() - t0, torch.cuda.max_memory_allocated() / 1e9))
    bb.release()


class BandedNormals:
    """model_normal [rows, cols, 4] as the restatement indexes it: `last` in the last row, bands[(row // 64) % 3] everywhere else"""

    def __init__(self, rows, bands, last):
        self.rows, self.bands, self.last = rows, np.asarray(bands, F), np.asarray(last, F)

    def __getitem__(self, index):
        vm = np.asarray(index[0])
        return np.where((vm == self.rows - 1)[:, None], self.last, self.bands[(vm // 64) % 3])


def unit(*n):
    n = np.asarray(n, np.float64)
    return np.append(n / np.linalg.norm(n), 1.0).astype(F)


def test_a_model_normal_image_past_4_gib(hip_ctx):
    import torch
    rows, cols, step = 16385, 16384, 64
    assert rows * cols * 16 > 1 << 32 and (rows - 1) * cols * 16 == 1 << 32 and (rows - 1) % step == 0
    bb.need_memory(8 * GB)
    camera = dict(fx=16000.0, fy=16000.0, cx=cols / 2 - 0.5, cy=16380.0)
    bands, last = np.stack([unit(0.1, 0.2, -1.0), unit(-0.3, 0.1, -1.0), unit(0.2, -0.3, -1.0)]), unit(-0.2, 0.1, -1.0)
    u = np.arange(cols)
    pattern = (2000 + (u * 7) % 41 - 20).astype(np.uint16)          # millimetres about the plane's 2 m
    pattern[(u // step) % 11 == 3] = 0                               # and samples that hold no depth
    X0 = cases.offset((0.01, 0.0, 0.0), (0.0, 0.002, 0.0))

    rp = ref.params(camera, "u16", 1e-3, max_iterations=2)
    p = ops.dense_align_params(camera, "u16", 1e-3, max_iterations=2)
    host = (np.broadcast_to(F(2.0), (rows, cols)), BandedNormals(rows, bands, last), np.broadcast_to(pattern, (rows, cols)))
    X, res, cls = ref.align(rp, X0, *host, None, step)
    n = ref.shape_of(rows, cols, step)[2]
    assert n == 257 * 256 == res["num_samples"] and res["steps_taken"] == 2 and res["num_inliers"] > 40000 and res["num_unmatched"] > 4000
    assert (cls.reshape(257, 256)[-1] == ref.INLIER).sum() > 100     # the last row's samples meet the model, past 2^32 bytes
    # and the last row's normal matters: with the other normal there the result is another one
    other = ref.align(rp, X0, host[0], BandedNormals(rows, bands, bands[1]), host[2], None, step)
    assert other[0].tobytes() != X.tobytes() and other[1]["H"].tobytes() != res["H"].tobytes()

    ab = ops.DenseAlignBatch(hip_ctx, 1, rows, cols, mask=True)
    model_depth = torch.full((1, rows, cols), 2.0, dtype=torch.float32, device="cuda")
    model_normal = torch.empty((1, rows, cols, 4), dtype=torch.float32, device="cuda")
    banded = model_normal[0, :rows - 1].view((rows - 1) // 64, 64, cols, 4)
    for k in range(3):
        banded[k::3] = torch.from_numpy(bands[k]).cuda()
    model_normal[0, rows - 1] = torch.from_numpy(last).cuda()
    live = torch.from_numpy(pattern.view(np.int16)).cuda()[None, None, :].expand(1, rows, cols).contiguous().view(torch.uint16)
    bb.fill_sentinel(ab.result, ab.mask)
    ab.X.copy_(torch.from_numpy(X0.reshape(1, 16)))
    ab.run(p, model_depth, model_normal, live, None, step)
    hip_ctx.synchronize()
    assert ab.X.cpu().numpy().tobytes() == X.tobytes()
    assert ab.results()[0].tobytes() == rig_.result_bytes(res)
    mask = ab.mask.cpu().numpy()
    assert mask[:n].tobytes() == cls.tobytes() and (mask[n:n + 4096] == bb.SENTINEL).all()
    assert int(torch.count_nonzero(ab.mask[n:] != bb.SENTINEL)) == 0
    del ab, model_depth, model_normal, live
