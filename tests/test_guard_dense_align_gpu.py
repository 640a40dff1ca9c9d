"""prs_dense_align_batch_run inside guard bands (tests/guarded.py) at the buffer sizes and alignments
include/proslam_hip_dense_align.h documents, as tests/test_guard_tsdf_raycast_gpu.py has the raycast.

Every caller-owned array of the call lies in an arena, at exactly the demanded alignment (a multiple of it, never of twice it), with a
band of fill bytes on either side and not one byte more than the header gives it: a depth image ends with the last pixel of its last
row, the workspace has the bytes the library's query answers, the normals have rows * cols rows of 16 bytes a pair, mask has
batch * N bytes.  A case runs with fill 0x00 and with fill 0xFF; both runs must equal the restatement, equal each other byte for byte
and leave every band clean.  What the call must not read -- the pitch padding of both depth images, the images of a pair whose estimate
is not finite -- holds the fill.  One case understates result's extent on purpose, to show that the harness reports a write behind it."""
import numpy as np
import pytest

import guarded
import dense_align_ref as ref
from dense_align_rig import Rig, pair_of, params_pair
from srrg2_proslam_amd import ops

pytestmark = pytest.mark.gpu
F = np.float32
ROWS, COLS = 41, 25       # two chunks a pair, the second of one sample


def run_case(hip_ctx, arena, pad, step=1, shrink=None):
    fill_f, fill_u = guarded.host_fill(F, arena.fill), guarded.host_fill(np.uint16, arena.fill)
    pairs = [pair_of(ROWS, COLS, "u16", seed) for seed in (30, 31, 32)]
    pairs[1]["X0"][0, 3] = np.inf                        # nothing of this pair is read but its estimate
    pairs[1].update(model_depth=np.full((ROWS, COLS), fill_f, F), model_normal=np.full((ROWS, COLS, 4), fill_f, F),
                    live_depth=np.full((ROWS, COLS), fill_u, np.uint16), live_normal=np.full((ROWS, COLS, 4), fill_f, F))

    def take(shape, dtype, align, name):
        extent = None
        if name in ("model_depth", "live_depth"):  # ends with the last pixel of the last row
            extent = (int(np.prod(shape)) - pad) * (4 if name == "model_depth" else 2)
        if name == shrink:
            extent = int(np.prod(shape)) * 4 - 8
        return arena.take(shape, dtype, align, name, extent=extent)

    r = Rig(hip_ctx, pairs, step, pad, pad, take=take)
    r.upload(slack=(fill_f, fill_u))
    want = r.check(*params_pair(ops, pairs[0], max_iterations=3))
    assert [w[1]["warnings"] for w in want] == [0, ref.PRS_ERR_RANGE, 0]
    assert want[1][1]["steps_taken"] == 0 and min(want[0][1]["steps_taken"], want[2][1]["steps_taken"]) >= 2
    assert min(want[2][1][k] for k in ("num_unmatched", "num_inliers", "num_rejected", "num_invalid")) > 0
    return r.outputs()


@pytest.mark.parametrize("pad,step", [(0, 1), (1, 1), (3, 2)])
def test_dense_align(hip_ctx, pad, step):
    guarded.both_fills(lambda arena: run_case(hip_ctx, arena, pad, step))


def test_an_understated_extent_is_reported(hip_ctx):
    """the harness believes result to end 8 bytes early: the last pair's reserved words land in the band"""
    arena = guarded.Arena(0xFF)  # whatever the call stores there, zeros included, is not the fill
    run_case(hip_ctx, arena, 0, shrink="result")
    with pytest.raises(guarded.Violation) as report:
        arena.check()
    assert "result" in str(report.value) and "after" in str(report.value)
