"""prs_tsdf_raycast_batch_run inside guard bands (tests/guarded.py) at the buffer sizes and alignments
include/proslam_hip_tsdf_raycast.h documents, as tests/test_guard_tsdf_gpu.py has the fusion.

Every caller-owned array of the call lies in an arena, at exactly the demanded alignment (a multiple of it, never of twice it), with a
band of fill bytes on either side and not one byte more than the header gives it: depth ends with the last pixel of the last row of the
last view, the workspace has the bytes the library's query answers, normal has rows * cols rows of 16 bytes a view.  A case runs with
fill 0x00 and with fill 0xFF; both runs must equal the restatement, equal each other byte for byte and leave every band clean.  What the
call must not read -- the volume of a refused sequence, the indices of the views from n_views on, the poses no view names -- holds the
fill.  One case understates normal's extent on purpose, to show that the harness reports a write behind it."""
import numpy as np
import pytest

import guarded
import tsdf_raycast_ref as ref
from tsdf_raycast_rig import OUTPUTS, Rig, fused, params_pair, views_of
from srrg2_proslam_amd import ops

pytestmark = pytest.mark.gpu
F = np.float32
DIMS, VIEWS = (33, 5, 9), 3
N_VIEWS = (1, 7, VIEWS)        # the second sequence is refused, the last is the full one


def run_case(hip_ctx, arena, pad, shrink=None):
    made = [fused((2, b) + DIMS, DIMS) for b in range(3)]
    seqs = [views_of((31, b), VIEWS, VIEWS + 1, index=True, n_views=n) for b, n in enumerate(N_VIEWS)]
    fill_f, fill_i = guarded.host_fill(F, arena.fill), guarded.host_fill(np.int32, arena.fill)
    volumes = [m[0] for m in made]
    volumes[1] = np.full_like(volumes[1], fill_f)           # the refused sequence's volume is not read
    seqs[1]["pose"][:] = fill_f
    seqs[1]["view_index"][:] = fill_i
    seqs[0]["view_index"][1:] = fill_i                      # the views from n_views on have no index
    for s in (seqs[0], seqs[2]):
        named = set(s["view_index"][:s["n_views"]].tolist())
        for k in range(VIEWS + 1):
            if k not in named:
                s["pose"][k] = fill_f                       # a pose no view names

    def take(shape, dtype, align, name):
        extent = None
        if name == "depth":  # ends with the last pixel of the last row
            extent = ((int(np.prod(shape[:-1])) - 1) * shape[-1] + shape[-1] - pad) * 4
        if name == shrink:
            extent = int(np.prod(shape)) * 4 - 16
        return arena.take(shape, dtype, align, name, extent=extent)

    r = Rig(hip_ctx, volumes, [m[1] for m in made], seqs, VIEWS, pad=pad, take=take)
    want = r.check(*params_pair(ops))
    assert [w["status"] for w in want] == [0, ref.PRS_ERR_RANGE, 0] and want[2]["n_hit"].min() > 50 and want[0]["n_hit"][0] > 50
    return {k: r.get(k) for k in OUTPUTS}


@pytest.mark.parametrize("pad", [0, 1])
def test_tsdf_raycast(hip_ctx, pad):
    guarded.both_fills(lambda arena: run_case(hip_ctx, arena, pad))


def test_an_understated_extent_is_reported(hip_ctx):
    """the harness believes normal to end 16 bytes early: the last pixel's store lands in the band"""
    arena = guarded.Arena(0xFF)  # whatever the call stores there, zeros included, is not the fill
    run_case(hip_ctx, arena, 0, shrink="normal")
    with pytest.raises(guarded.Violation) as report:
        arena.check()
    assert "normal" in str(report.value) and "after" in str(report.value)
