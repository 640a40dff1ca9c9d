"""prs_tsdf_integrate_batch_run and prs_tsdf_surface_batch_run inside guard bands (tests/guarded.py) at the buffer sizes and
alignments include/proslam_hip_tsdf.h documents, as tests/test_guard_normals_gpu.py has the depth normals.

Every caller-owned array of the two calls lies in an arena, at exactly the demanded alignment (a multiple of it, never of twice it),
with a band of fill bytes on either side and not one byte more than the header gives it: depth ends with the last pixel of the last
row of the last image, the workspaces have the bytes the library's queries answer, xyz, normal and cell have out_stride rows, and
out_stride is the number of crossings of the last sequence, so its last row adjoins a band.  A case runs with fill 0x00 and with
fill 0xFF; both runs must equal the restatement, equal each other byte for byte and leave every band clean.  What the calls must not
read -- the pitch padding, the images from n_images on, the volume of a refused sequence -- holds the fill.  One case understates an
extent on purpose, to show that the harness reports a write behind it."""
import numpy as np
import pytest

import guarded
import tsdf_ref as ref
from tsdf_rig import Rig, origin_in_front, params_pair, scene
from srrg2_proslam_amd import ops

pytestmark = pytest.mark.gpu
F = np.float32
DIMS, FRAMES = (33, 5, 9), 3   # ragged bricks, two chunks of voxels
N_IMAGES = (1, 7, FRAMES)      # the second sequence is refused, the last is the full one


def build(depth_type):
    """the host side: the sequences, their origins and the crossings of the last sequence"""
    seqs = [scene((31, b), DIMS, FRAMES, depth_type, n_images=n, index=True, pose_stride=FRAMES + 1) for b, n in enumerate(N_IMAGES)]
    origins = [origin_in_front(DIMS, shift=(0.01 * b, 0.0)) for b in range(3)]
    _, rp = params_pair(ops, depth_type)
    last = ref.integrate(seqs[2], rp, origins[2], np.zeros((DIMS[2], DIMS[1], DIMS[0], 2), F))
    cap = ref.surface(last["volume"], rp, origins[2], 0, count_only=True)["n_total"]
    assert cap > 30
    return seqs, origins, cap


def run_case(hip_ctx, arena, depth_type, pad, shrink=None):
    seqs, origins, cap = build(depth_type)
    es = 2 if depth_type == "u16" else 4
    np_dtype = np.uint16 if depth_type == "u16" else F

    def take(shape, dtype, align, name):
        extent = None
        if name == "depth":  # ends with the last pixel of the last row
            extent = (int(np.prod(shape[:-1]) - 1) * shape[-1] + shape[-1] - pad) * es
        if name == shrink:
            extent = int(np.prod(shape)) * 4 - 16
        return arena.take(shape, dtype, align, name, extent=extent)

    r = Rig(hip_ctx, seqs, origins, DIMS, depth_type, pad, out_stride=cap, take=take)
    r.upload(seqs, slack=guarded.host_fill(np_dtype, arena.fill))
    p, rp = params_pair(ops, depth_type)
    before = np.zeros((3, DIMS[2], DIMS[1], DIMS[0], 2), F)
    before[1] = guarded.host_fill(F, arena.fill)  # the refused sequence's volume is neither read nor written
    want = r.check_integrate(p, rp, before)
    assert [w["status"] for w in want] == [0, ref.PRS_ERR_RANGE, 0] and want[2]["n_updates"].min() > 100
    volume = r.get("volume")
    volume[1] = 0  # an empty volume in the refused sequence's place: the surface call reads every volume
    surface = r.check_surface(p, rp, volume)
    assert surface[2]["n_out"] == surface[2]["n_total"] == cap and surface[2]["status"] == 0
    return {k: r.get(k) for k in ("volume", "n_updates", "n_skipped", "status", "xyz", "normal", "cell", "n_out", "n_total", "surface_status")}


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("depth_type", ["u16", "f32"])
def test_tsdf(hip_ctx, depth_type, pad):
    guarded.both_fills(lambda arena: run_case(hip_ctx, arena, depth_type, pad))


@pytest.mark.parametrize("name", ["xyz", "normal"])
def test_an_understated_extent_is_reported(hip_ctx, name):
    """the harness believes the array to end 16 bytes early: the last crossing's store lands in the band"""
    arena = guarded.Arena(0xFF)  # whatever the call stores there, zeros included, is not the fill
    run_case(hip_ctx, arena, "f32", 0, shrink=name)
    with pytest.raises(guarded.Violation) as report:
        arena.check()
    assert name in str(report.value) and "after" in str(report.value)
