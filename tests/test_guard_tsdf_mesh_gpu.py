"""prs_tsdf_mesh_batch_run inside guard bands (tests/guarded.py) at the buffer sizes and alignments
include/proslam_hip_tsdf_mesh.h documents, as tests/test_guard_tsdf_raycast_gpu.py has the raycast.

Every caller-owned array of the call lies in an arena, at exactly the demanded alignment (a multiple of it, never of twice it), with a
band of fill bytes on either side and not one byte more than the header gives it: vertex and normal have vertex_stride rows of 16 bytes
a sequence, quad quad_stride rows of 16 bytes, cube and edge one int32 a row, the workspace the bytes the library's query answers.  A
case runs with fill 0x00 and with fill 0xFF; both runs must equal the restatement, equal each other byte for byte and leave every band
clean.  The workspace starts as the fill in either run: the rank map in it is not cleared by the call, which reads it only where it
has written it, so a rank that came out of the fill would differ between the two runs.  The batch holds a sequence that overflows both
strides, whose rows end exactly at the band.  One case understates quad's extent on purpose, to show that the harness reports a write
behind it."""
import numpy as np
import pytest

import guarded
import tsdf_mesh_rig as rig_
import tsdf_ref
from tsdf_mesh_rig import COUNTS, ROWS, Rig, host_params
from tsdf_rig import K
from srrg2_proslam_amd import ops

pytestmark = pytest.mark.gpu
F = np.float32
DIMS = (70, 9, 6)              # four chunks, the last one ragged
NV, NQ = 184, 153              # the plane's mesh at that size


def run_case(hip_ctx, arena, shrink=None):
    plane, origin = rig_.plane_volume(DIMS)
    noise, _ = rig_.random_volume(DIMS, 6)     # overflows both strides
    empty, _ = rig_.empty_volume(DIMS)
    assert rig_.totals(rig_.plane_volume, DIMS) == (NV, NQ)
    assert min(rig_.totals(rig_.random_volume, DIMS, 6)) > max(NV, NQ)

    def take(shape, dtype, align, name):
        extent = int(np.prod(shape)) * 4 - 16 if name == shrink else None
        return arena.take(shape, dtype, align, name, extent=extent)

    r = Rig(hip_ctx, [plane, noise, empty, plane], [origin] * 4, NV, NQ, take=take)
    p = ops.tsdf_params(K, voxel_size=rig_.VS, truncation=rig_.TRUNC, min_weight=1.0)
    want = r.check(p, host_params(), "guarded")
    assert [w["status"] for w in want] == [0, tsdf_ref.PRS_ERR_CAPACITY, 0, 0]
    assert [(w["n_vertices"], w["n_quads"]) for w in want] == [(NV, NQ), (NV, NQ), (0, 0), (NV, NQ)]
    return {k: r.get(k) for k in ROWS + COUNTS}


def test_tsdf_mesh(hip_ctx):
    guarded.both_fills(lambda arena: run_case(hip_ctx, arena))


def test_an_understated_extent_is_reported(hip_ctx):
    """the harness believes quad to end 16 bytes early: the last sequence's last row lands in the band"""
    arena = guarded.Arena(0xFF)  # whatever the call stores there is not the fill: a rank is never -1 in all four words
    run_case(hip_ctx, arena, shrink="quad")
    with pytest.raises(guarded.Violation) as report:
        arena.check()
    assert "quad" in str(report.value) and "after" in str(report.value)
