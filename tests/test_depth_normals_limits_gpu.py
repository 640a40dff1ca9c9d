"""Depth normals at the two things that only exist at the batch sizes the stage is built for, as tests/test_dense_limits_gpu.py has
them for the other dense stages (whose Stage rig and helpers are reused, with tests/big_batch.py).

A. The launch-size guard.  With 1 x 1 images the tile launch has one workgroup an image: at batch * frames = 2^24 - 1 the call runs
   and is right, with one sequence more it returns PRS_ERR_UNSUPPORTED and has written nothing.
B. normal past 2^32 bytes.  16 bytes a pixel, so 2^28 pixels: small images, periodic input, compared over its whole length, the
   images a call must not touch (at the highest addresses) included.

Out of scope: row_normal, which passes 2^32 bytes only with 2^28 cloud rows and their 2^28 frames and pixels beside the images."""
import ctypes as C
import time

import numpy as np
import pytest

import big_batch as bb
import depth_normals_cases as cases
import depth_normals_ref as ref
import test_dense_limits_gpu as limits
from srrg2_proslam_amd import _lib, _lib_normals, ops

pytestmark = pytest.mark.gpu
F = np.float32
FRAMES, LIMIT, GB = limits.FRAMES, limits.LIMIT, limits.GB
K = cases.K


@pytest.fixture(autouse=True)
def report():
    """prints what the test took: seconds and the peak of device memory"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print("\n[depth normals limits] %.1f s, peak %.2f GB of device memory" % (time.time() - t0, torch.cuda.max_memory_allocated() / 1e9))
    bb.release()


class Normals(limits.Stage):
    """float32 depth with `pad` valid elements behind every row"""

    def __init__(self, ctx, B, rows, cols, pad=0, radius=2, smooth=1, frames=FRAMES):
        self.ctx, S = ctx, self.P + 2
        self.t_n = self.n_images(B, frames)
        depth = cases.random_depth(np.random.default_rng([81, rows, cols]), (S, frames, rows, cols), "f32")
        self.nb = ops.DepthNormalsBatch(B, frames, rows, cols)
        self.p, rp = ops.depth_normals_params(K, radius, smooth, depth_type="f32"), ref.params(K, radius, smooth)
        full = np.full((S, frames, rows, cols + pad), 2.0, F)
        full[..., :cols] = depth
        self.t_depth = bb.periodic(full[:self.P], B, full[self.P:])
        self.t = dict(normal=self.nb.normal, n_normal=self.nb.n_normal, status=self.nb.status)
        self.cols, self.inplace = cols, {}
        before = dict(normal=bb.sentinel((frames, rows, cols, 4), F), n_normal=bb.sentinel((frames,), np.int32))
        results = [ref.depth_normals(dict(depth=depth[s], n_images=self.n_host[s]), rp, before) for s in range(S)]
        self.want = dict(normal=np.stack([r["normal"] for r in results]), n_normal=np.stack([r["n_normal"] for r in results]),
                         status=np.array([r["status"] for r in results], np.int32))
        self.found = int(sum(r["n_normal"][:n].sum() for r, n in zip(results, self.n_host)))

    def call(self):
        d = self.nb.descriptor(self.p, self.t_depth[..., :self.cols], n_images=self.t_n)
        return _lib_normals.load().prs_depth_normals_batch_run(self.ctx._h, C.byref(self.p), C.byref(d))


# ---- A. the launch-size guard ----------------------------------------------------------------------------------------------------------
def test_the_largest_launch_that_fits_runs_and_is_right(hip_ctx):
    assert _lib.load().prs_launch_fits(LIMIT, 256) == 1 and limits.SEQUENCES * FRAMES == LIMIT
    bb.need_memory(2 * GB)
    rig = Normals(hip_ctx, limits.SEQUENCES, 1, 1)
    rig.fill()
    assert rig.call() == 0
    rig.compare("depth normals")
    del rig


def test_one_more_is_refused_and_nothing_is_written(hip_ctx):
    assert _lib.load().prs_launch_fits(LIMIT + 1, 256) == 0
    bb.need_memory(2 * GB)
    rig = Normals(hip_ctx, limits.SEQUENCES + 1, 1, 1)
    rig.fill()
    assert rig.call() == limits.UNSUPPORTED
    rig.compare_untouched("depth normals")
    del rig


# ---- B. normal past 2^32 bytes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [(2, 1), (8, 0)], ids=lambda s: "r%d_s%d" % s)
def test_normal_past_4_gib(hip_ctx, setting):
    B = limits.sequences_for(1 << 28)
    bb.need_memory(8 * GB)
    rig = Normals(hip_ctx, B, limits.ROWS, limits.COLS, pad=1, radius=setting[0], smooth=setting[1])
    limits.crossing(rig, (("normal", limits.PIXELS * 16, None),), "depth normals")
    assert rig.t_depth.stride(2) == limits.COLS + 1 and rig.found > 300  # over the 19 served images of the period; radius 8 finds few
    rig.fill()
    assert rig.call() == 0
    rig.compare("depth normals past 4 GiB")
    del rig
