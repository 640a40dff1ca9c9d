"""The launch-size rule at the entry points that launch one workgroup a sequence, image or map (tests/test_dense_limits_gpu.py has
the dense stages).  HIP takes no launch of 2^32 or more work-items, 2^24 - 1 workgroups of 256 threads (prs_launch_fits,
tests/test_launch_fits.py), so a batch of 2^24 is one too many: the call returns PRS_ERR_UNSUPPORTED before it has enqueued or
written anything.

Every array is allocated for the declared batch, with the smallest strides the entry point takes, and holds the sentinel in every
byte, inputs included: a call that did launch would stay inside its buffers, and would be seen in the outputs.  No kernel runs."""
import ctypes as C
import time

import numpy as np
import pytest

import big_batch as bb
from tests import merge_cases as mc
from srrg2_proslam_amd import _lib
from test_merge_dispatch_gpu import gpu_params

pytestmark = pytest.mark.gpu
UNSUPPORTED = -5
B = 1 << 24
GB = 1 << 30


def dev(*shape, dtype=np.float32):
    """a device array of the shape (first dimension: the batch) with the sentinel in every byte"""
    import torch
    t = torch.empty(shape + (np.dtype(dtype).itemsize,), dtype=torch.uint8, device="cuda")
    bb.fill_sentinel(t)
    return t


def scene_clip(ctx, n=B):
    """the walk shape (128 scenes or more): one workgroup walks a scene of `stride` = 1 points"""
    t = dict(scene_xyzw=dev(n, 1, 4), n_scene=dev(n, dtype=np.int32), robot_in_local_map=dev(n, 16), clipped_xyzw=dev(n, 1, 4),
             global_indices=dev(n, 1, dtype=np.int32), n_clipped=dev(n, dtype=np.int32), status=dev(n, dtype=np.int32))
    d = _lib.ClipBatch(batch=n, stride=1, **{k: v.data_ptr() for k, v in t.items()})
    projector = _lib.Projector(500.0, 500.0, 320.0, 240.0, 640, 480, 0.1, 50.0)
    S = np.eye(4, dtype=np.float32).reshape(16)
    return t, lambda: _lib.load().prs_scene_clip_batch(ctx._h, C.byref(projector), S.ctypes.data, C.byref(d))


def merge(ctx):
    """the weighted-mean merger, one kernel of one workgroup a map: maps of one landmark, one pose-table row and no history, frames
    of one measurement and one correspondence"""
    i32, u8 = np.int32, np.uint8
    t = dict(coords=dev(B, 1, 4), desc=dev(B, 1, 32, dtype=u8), state=dev(B, 1, 4), covariance=dev(B, 1, 9), n_opt=dev(B, 1, dtype=i32),
             inlier=dev(B, 1, dtype=u8), n_meas=dev(B, 1, dtype=i32), poses=dev(B, 1, 24), n_points=dev(B, dtype=i32),
             measurement=dev(B, 1, 4), measurement_desc=dev(B, 1, 32, dtype=u8), n_measured=dev(B, dtype=i32), corr=dev(B, 1, 3),
             n_corr=dev(B, dtype=i32), measurement_in_world=dev(B, 16), measurement_in_scene=dev(B, 16), frame=dev(B, dtype=i32),
             result=dev(B, 3, dtype=i32))
    assert C.sizeof(_lib.MergeResult) == 12 and t["poses"][0].numel() == 96 and t["corr"][0].numel() == 12  # prs_frame_pose, prs_corr
    d = _lib.MergeBatch(batch=B, capacity=1, max_measurements=0, max_frames=1, measurement_stride=1, corr_stride=1,
                        **{k: v.data_ptr() for k, v in t.items()})
    p = gpu_params(mc.merger_params("weighted_mean", 1))
    return t, lambda: _lib.load().prs_merge_batch_run(ctx._h, C.byref(p), C.byref(d))


def extract_features(ctx):
    """the smallest image, 7 x 7, and one feature an image: the selection and the descriptor launches have a workgroup an image"""
    t = dict(images=dev(B, 7, 7, dtype=np.uint8), keypoints=dev(B, 1, 2), descriptors=dev(B, 1, 32, dtype=np.uint8),
             n_features=dev(B, dtype=np.int32), status=dev(B, dtype=np.int32))
    d = _lib.ExtractBatch(batch=B, rows=7, cols=7, pitch=7, stride=1, **{k: v.data_ptr() for k, v in t.items()})
    p = _lib.ExtractorParams(detector_threshold=20, enable_non_maximum_suppression=1, target_number_of_keypoints=1, number_of_detectors_vertical=1,
                             number_of_detectors_horizontal=1, selection_order=0, max_raw_detections=0)
    return t, lambda: _lib.load().prs_extract_features_batch(ctx._h, C.byref(p), C.byref(d))


RIGS = dict(scene_clip=scene_clip, merge=merge, extract_features=extract_features)
MEMORY = dict(scene_clip=3 * GB, merge=9 * GB, extract_features=3 * GB)  # the rigs hold 1.9, 7.1 and 1.6 GB


@pytest.mark.parametrize("entry", sorted(RIGS))
def test_a_batch_of_2_to_the_24_is_refused_and_nothing_is_written(hip_ctx, entry):
    import torch
    assert _lib.load().prs_launch_fits(B - 1, 256) == 1 and _lib.load().prs_launch_fits(B, 256) == 0
    bb.need_memory(MEMORY[entry])
    torch.cuda.synchronize()
    t0 = time.time()
    arrays, call = RIGS[entry](hip_ctx)
    assert call() == UNSUPPORTED
    message = _lib.load().prs_last_error(hip_ctx._h).decode()
    assert message.endswith(": more work-items than one launch holds") and message.startswith("prs_"), message
    torch.cuda.synchronize()
    bb.compare_sentinel(entry, *arrays.values())
    print("\n[launch limits] %s: %.1f s, %.2f GB of device memory" % (entry, time.time() - t0, sum(a.numel() for a in arrays.values()) / 1e9))
    del arrays, call
    bb.release()


def test_the_scene_clipper_runs_at_a_batch_that_fits(hip_ctx):
    """the refusal above is the limit's, not the rig's: the scene clipper's rig at 128 scenes, still the walk shape, is taken.
    Scenes of n_scene < 0 (the sentinel) are empty: PRS_WARN_EMPTY_INPUT, and outputs and n_clipped untouched"""
    t, call = scene_clip(hip_ctx, 128)
    assert call() == 0
    hip_ctx.synchronize()
    status = t["status"].view(-1).cpu().numpy().view(np.int32)
    assert (status == _lib.WARN_EMPTY_INPUT).all(), status[:4]
    bb.compare_sentinel("scene clip, empty scenes", t["clipped_xyzw"], t["global_indices"], t["n_clipped"])
