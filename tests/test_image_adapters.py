"""The Python adapters of the dense image stages (ops.DepthCloudBatch, DenseStereoBatch, SgmStereoBatch, SpeckleFilterBatch,
DepthConsistencyBatch) on CPU tensors: the descriptor each builds from a dense tensor, from a view of longer rows and from the
[B * F, rows, cols] form, the inputs each refuses, and the boundary values the two stereo parameter builders refuse.  No kernel
runs: the batches are built with device=torch.device("cpu") and only their descriptors are read.  (RectifyBatch takes a context
and allocates on the GPU: tests/test_rectify_gpu.py has it.)"""
import numpy as np
import pytest
import torch

from srrg2_proslam_amd import ops

CPU = torch.device("cpu")
B, F, ROWS, COLS, PITCH = 2, 2, 3, 5, 8
CAMERA = {"fx": 500.0, "fy": 500.0, "cx": 2.0, "cy": 1.0, "baseline_m": 0.5}


def dense(dtype, shape=(B, F, ROWS, COLS)):
    return torch.zeros(shape, dtype=dtype)


def pitched(dtype):
    """[B, F, ROWS, COLS] view of rows of PITCH elements"""
    return torch.zeros((B, F, ROWS, PITCH), dtype=dtype)[..., :COLS]


def flat(dtype):
    return torch.zeros((B * F, ROWS, COLS), dtype=dtype)


def strided(dtype):
    """inner stride 2"""
    return torch.zeros((B, F, ROWS, 2 * COLS), dtype=dtype)[..., ::2]


def gapped(dtype):
    """images that do not follow one another at rows * pitch"""
    return torch.zeros((B, F, ROWS + 1, COLS), dtype=dtype)[:, :, :ROWS]


def i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def sizes(d):
    return d.batch, d.frames, d.rows, d.cols


def refused(call, *args, **kwargs):
    with pytest.raises(ValueError):
        call(*args, **kwargs)


# ---- the two stereo adapters: one descriptor layout but for images_in_flight ----
STEREO = [(ops.DenseStereoBatch, {}), (ops.SgmStereoBatch, {"images_in_flight": 3})]


@pytest.mark.parametrize("cls, more", STEREO, ids=["dense", "sgm"])
def test_stereo_descriptor(cls, more):
    batch = cls(B, F, ROWS, COLS, device=CPU, **more)
    assert batch.out_pitch == 32 and tuple(batch._disparity.shape) == (B, F, ROWS, 8) and tuple(batch.disparity.shape) == (B, F, ROWS, COLS)
    assert batch.disparity.data_ptr() == batch._disparity.data_ptr() and batch.depth.data_ptr() == batch._depth.data_ptr()
    left, right, n = dense(torch.uint8), pitched(torch.uint8), i32(B)
    d = batch.descriptor(left, right, n)
    assert sizes(d) == (B, F, ROWS, COLS) and (d.left_pitch, d.right_pitch, d.out_pitch) == (COLS, PITCH, 32)
    assert (d.left, d.right, d.n_images) == (left.data_ptr(), right.data_ptr(), n.data_ptr())
    assert (d.disparity, d.depth, d.n_valid) == (batch._disparity.data_ptr(), batch._depth.data_ptr(), batch.n_valid.data_ptr())
    assert (d.status, d.workspace) == (batch.status.data_ptr(), batch.workspace.data_ptr())
    if more:
        assert d.images_in_flight == 3 == batch.images_in_flight
    d = batch.descriptor(flat(torch.uint8), flat(torch.uint8))
    assert (d.left_pitch, d.right_pitch) == (COLS, COLS) and d.n_images is None
    only = cls(B, F, ROWS, COLS, outputs=("depth",), device=CPU)
    d = only.descriptor(left, right)
    assert only.disparity is None and only.n_valid is None and (d.disparity, d.n_valid) == (None, None) and d.depth == only._depth.data_ptr()


@pytest.mark.parametrize("cls, more", STEREO, ids=["dense", "sgm"])
def test_stereo_refusals(cls, more):
    batch = cls(B, F, ROWS, COLS, device=CPU, **more)
    good = dense(torch.uint8)
    for bad in (dense(torch.uint16), strided(torch.uint8), gapped(torch.uint8), dense(torch.uint8, (B, F, ROWS, COLS + 1)),
                dense(torch.uint8, (B * F, ROWS + 1, COLS))):
        refused(batch.descriptor, bad, good)
        refused(batch.descriptor, good, bad)
    for n in (i32(B + 1), i32(B, 1), torch.zeros(B, dtype=torch.int64), i32(2 * B)[::2]):
        refused(batch.descriptor, good, good, n)
    refused(cls, B, F, ROWS, COLS, outputs=("disparity", "labels"), device=CPU)
    refused(cls, B, F, ROWS, COLS, outputs=("n_valid",), device=CPU)
    for shape in ((0, F, ROWS, COLS), (B, 0, ROWS, COLS), (B, F, 0, COLS), (B, F, ROWS, 0)):
        refused(cls, *shape, device=CPU)


def test_sgm_batch_refusals():
    refused(ops.SgmStereoBatch, B, F, ROWS, COLS, images_in_flight=0, device=CPU)
    refused(ops.SgmStereoBatch, B, F, ROWS, COLS, n_disparities=257, device=CPU)
    assert ops.SgmStereoBatch(B, F, ROWS, COLS, images_in_flight=9, device=CPU).images_in_flight == B * F


# ---- the speckle filter ----
def test_speckle_descriptor():
    batch = ops.SpeckleFilterBatch(B, F, ROWS, COLS, outputs=ops.SpeckleFilterBatch.OUTPUTS, device=CPU)
    assert batch.label_pitch == 32 and tuple(batch._label.shape) == (B, F, ROWS, 8) and batch.label.data_ptr() == batch._label.data_ptr()
    p = ops.speckle_params(pixel_type="f32", companion_type="u16")
    image, companion, n = pitched(torch.float32), dense(torch.uint16), i32(B)
    d = batch.descriptor(p, image, companion, n)
    assert sizes(d) == (B, F, ROWS, COLS) and (d.pitch, d.companion_pitch, d.label_pitch) == (4 * PITCH, 2 * COLS, 32)
    assert (d.image, d.companion, d.n_images, d.label) == (image.data_ptr(), companion.data_ptr(), n.data_ptr(), batch._label.data_ptr())
    assert (d.n_kept, d.n_removed) == (batch.n_kept.data_ptr(), batch.n_removed.data_ptr())
    assert (d.status, d.workspace) == (batch.status.data_ptr(), batch.workspace.data_ptr())
    d = batch.descriptor(p, flat(torch.float32))
    assert d.pitch == 4 * COLS and (d.companion, d.companion_pitch, d.n_images) == (None, 0, None)
    plain = ops.SpeckleFilterBatch(B, F, ROWS, COLS, device=CPU)
    d = plain.descriptor(ops.speckle_params(pixel_type="u16"), dense(torch.uint16))
    assert plain.label is None and (d.label, d.label_pitch, d.pitch) == (None, 0, 2 * COLS)


def test_speckle_refusals():
    batch = ops.SpeckleFilterBatch(B, F, ROWS, COLS, device=CPU)
    p = ops.speckle_params(pixel_type="f32", companion_type="u16")
    good = dense(torch.float32)
    for bad in (dense(torch.uint16), strided(torch.float32), gapped(torch.float32), dense(torch.float32, (B, F, ROWS, COLS + 1))):
        refused(batch.descriptor, p, bad)
    for bad in (dense(torch.float32), strided(torch.uint16), gapped(torch.uint16)):
        refused(batch.descriptor, p, good, bad)
    for n in (i32(B + 1), i32(B, 1), torch.zeros(B, dtype=torch.int64), i32(2 * B)[::2]):
        refused(batch.descriptor, p, good, None, n)
    refused(ops.SpeckleFilterBatch, B, F, ROWS, COLS, outputs=("label", "n_valid"), device=CPU)
    for shape in ((0, F, ROWS, COLS), (B, 0, ROWS, COLS), (B, F, 0, COLS), (B, F, ROWS, 0)):
        refused(ops.SpeckleFilterBatch, *shape, device=CPU)


# ---- the dense cloud ----
def test_depth_cloud_descriptor():
    batch = ops.DepthCloudBatch(B, F, ROWS, COLS, 7, device=CPU)
    depth, gray, pose, n, index = dense(torch.uint16), pitched(torch.uint8), torch.zeros((B, 4, 16)), i32(B), i32(B, F)
    d = batch.descriptor(depth, pose, n, index, gray)
    assert sizes(d) == (B, F, ROWS, COLS) and (d.pitch, d.gray_pitch, d.pose_stride, d.out_stride) == (2 * COLS, PITCH, 4, 7)
    assert (d.depth, d.gray, d.pose, d.n_images, d.frame_index) == (depth.data_ptr(), gray.data_ptr(), pose.data_ptr(), n.data_ptr(), index.data_ptr())
    assert (d.xyz, d.frame, d.pixel, d.n_base) == (batch.xyz.data_ptr(), batch.node.data_ptr(), batch.row.data_ptr(), None)
    assert (d.n_out, d.n_total, d.n_skipped) == (batch.n_out.data_ptr(), batch.n_total.data_ptr(), batch.n_skipped.data_ptr())
    assert (d.status, d.workspace) == (batch.status.data_ptr(), batch.workspace.data_ptr())
    d = batch.descriptor(pitched(torch.float32), pose, n, append=True, count_only=True)
    assert d.pitch == 4 * PITCH and (d.gray, d.gray_pitch, d.frame_index, d.xyz, d.frame, d.pixel) == (None, 0, None, None, None, None)
    assert d.n_base == batch.n_out.data_ptr()
    bare = ops.DepthCloudBatch(B, F, ROWS, COLS, 7, outputs=(), device=CPU)
    d = bare.descriptor(depth, pose, n)
    assert bare.node is None and bare.row is None and (d.frame, d.pixel) == (None, None) and d.xyz == bare.xyz.data_ptr()
    # the adapter looks at neither the type of depth nor that of frame_index (the library is handed params.depth_type)
    batch.descriptor(dense(torch.float64), pose, n, torch.zeros((B, F), dtype=torch.int64))


def test_depth_cloud_refusals():
    batch = ops.DepthCloudBatch(B, F, ROWS, COLS, 7, device=CPU)
    good, pose, n = dense(torch.uint16), torch.zeros((B, 4, 16)), i32(B)
    for bad in (strided(torch.uint16), gapped(torch.uint16), flat(torch.uint16), dense(torch.uint16, (B, F, ROWS, COLS - 1)),
                dense(torch.uint16, (B, F + 1, ROWS, COLS))):
        refused(batch.descriptor, bad, pose, n)
    for bad in (strided(torch.uint8), gapped(torch.uint8), dense(torch.uint8, (B, F, ROWS, COLS - 1))):
        refused(batch.descriptor, good, pose, n, None, bad)
    for bad in (torch.zeros((B, 4, 12)), torch.zeros((B + 1, 4, 16)), torch.zeros((B, 4, 32))[..., ::2]):
        refused(batch.descriptor, good, bad, n)
    for index in (i32(B, F + 1), i32(B * F), i32(B, 2 * F)[:, ::2]):
        refused(batch.descriptor, good, pose, n, index)
    refused(ops.DepthCloudBatch, B, F, ROWS, COLS, 7, outputs=("frame", "gray"), device=CPU)
    for shape in ((0, F, ROWS, COLS, 7), (B, 0, ROWS, COLS, 7), (B, F, 0, COLS, 7), (B, F, ROWS, 0, 7), (B, F, ROWS, COLS, 0)):
        refused(ops.DepthCloudBatch, *shape, device=CPU)


# ---- the depth consistency filter ----
def test_depth_consistency_descriptor():
    batch = ops.DepthConsistencyBatch(B, F, ROWS, COLS, 2, outputs=ops.DepthConsistencyBatch.OUTPUTS, device=CPU)
    assert batch.dtype == torch.uint16 and tuple(batch._out.shape) == (B, F, ROWS, 8) and batch.out.data_ptr() == batch._out.data_ptr()
    depth, pose, n, index = pitched(torch.uint16), torch.zeros((B, 4, 16)), i32(B), i32(B, F)
    d = batch.descriptor(depth, pose, n, index)
    assert sizes(d) == (B, F, ROWS, COLS) and (d.pitch, d.out_pitch, d.count_pitch, d.pose_stride) == (2 * PITCH, 16, 8, 4)
    assert (d.depth, d.pose, d.n_images, d.frame_index, d.out) == (depth.data_ptr(), pose.data_ptr(), n.data_ptr(), index.data_ptr(), batch._out.data_ptr())
    assert (d.support, d.violation) == (batch._support.data_ptr(), batch._violation.data_ptr())
    assert (d.n_kept, d.n_removed, d.n_skipped) == (batch.n_kept.data_ptr(), batch.n_removed.data_ptr(), batch.n_skipped.data_ptr())
    assert (d.status, d.workspace) == (batch.status.data_ptr(), batch.workspace.data_ptr())
    plain = ops.DepthConsistencyBatch(B, F, ROWS, COLS, 1, depth_type="f32", device=CPU)
    d = plain.descriptor(dense(torch.float32), pose)
    assert (d.pitch, d.out_pitch, d.count_pitch) == (4 * COLS, 32, 8) and plain.support is None and plain.n_skipped is None
    assert (d.n_images, d.frame_index, d.support, d.violation, d.n_skipped) == (None, None, None, None, None)


def test_depth_consistency_refusals():
    batch = ops.DepthConsistencyBatch(B, F, ROWS, COLS, 2, device=CPU)
    good, pose = dense(torch.uint16), torch.zeros((B, 4, 16))
    for bad in (dense(torch.float32), strided(torch.uint16), gapped(torch.uint16), flat(torch.uint16), dense(torch.uint16, (B, F, ROWS, COLS - 1))):
        refused(batch.descriptor, bad, pose)
    for bad in (torch.zeros((B, 4, 12)), torch.zeros((B + 1, 4, 16)), torch.zeros((B, 4, 32))[..., ::2]):
        refused(batch.descriptor, good, bad)
    for n in (i32(B + 1), i32(B, 1), torch.zeros(B, dtype=torch.int64), i32(2 * B)[::2]):
        refused(batch.descriptor, good, pose, n)
    for index in (i32(B, F + 1), torch.zeros((B, F), dtype=torch.int64), i32(B, 2 * F)[:, ::2]):
        refused(batch.descriptor, good, pose, None, index)
    refused(ops.DepthConsistencyBatch, B, F, ROWS, COLS, 2, outputs=("support", "label"), device=CPU)
    refused(ops.DepthConsistencyBatch, B, F, ROWS, COLS, 2, depth_type="u8", device=CPU)
    refused(ops.DepthConsistencyBatch, B, F, ROWS, COLS, 2, depth_type=2, device=CPU)
    for window in (0, 9):
        refused(ops.DepthConsistencyBatch, B, F, ROWS, COLS, window, device=CPU)
    for shape in ((0, F, ROWS, COLS), (B, 0, ROWS, COLS), (B, F, 0, COLS), (B, F, ROWS, 0)):
        refused(ops.DepthConsistencyBatch, *shape, 2, device=CPU)


# ---- the parameter builders ----
@pytest.mark.parametrize("build", [ops.dense_stereo_params, ops.sgm_stereo_params], ids=["dense", "sgm"])
def test_stereo_params_boundaries(build):
    p = build(CAMERA, n_disparities=256, min_disparity=3840, uniqueness_percent=99, lr_max_diff=255)
    assert (p.n_disparities, p.min_disparity, p.uniqueness_percent, p.lr_max_diff) == (256, 3840, 99, 255)
    assert p.bf == float(np.float32(np.float64(CAMERA["fx"]) * np.float64(CAMERA["baseline_m"])))
    p = build(CAMERA, n_disparities=1, min_disparity=0, uniqueness_percent=0, lr_max_diff=-1)
    assert (p.n_disparities, p.uniqueness_percent, p.lr_max_diff) == (1, 0, -1)
    for bad in (dict(n_disparities=0), dict(n_disparities=257), dict(n_disparities=256, min_disparity=3841), dict(min_disparity=-1),
                dict(uniqueness_percent=100), dict(uniqueness_percent=-1), dict(lr_max_diff=-2), dict(lr_max_diff=256)):
        refused(build, CAMERA, **bad)
    for camera in ({"fx": 3e38, "baseline_m": 2.0}, {"fx": 500.0, "baseline_m": 0.0}, {"fx": 500.0, "baseline_m": -0.5},
                   {"fx": float("nan"), "baseline_m": 0.5}):
        refused(build, camera)


def test_stereo_params_own_fields():
    assert ops.dense_stereo_params(CAMERA, aggregation_radius=7).aggregation_radius == 7
    for radius in (-1, 8):
        refused(ops.dense_stereo_params, CAMERA, aggregation_radius=radius)
    p = ops.sgm_stereo_params(CAMERA, p1=0, p2=4095, n_paths=4)
    assert (p.p1, p.p2, p.n_paths) == (0, 4095, 4)
    for bad in (dict(p1=-1), dict(p1=11, p2=10), dict(p2=4096), dict(n_paths=6)):
        refused(ops.sgm_stereo_params, CAMERA, **bad)


def test_depth_type_parsing():
    assert ops.depth_cloud_params(CAMERA, depth_type="f32").depth_type == ops.DEPTH_F32
    assert ops.depth_cloud_params(CAMERA, depth_type=7).depth_type == 7  # an integer goes to the library, which refuses it
    refused(ops.depth_cloud_params, CAMERA, depth_type="u8")
    assert ops.depth_consistency_params(CAMERA, depth_type=ops.DEPTH_U16).depth_type == ops.DEPTH_U16
    refused(ops.depth_consistency_params, CAMERA, depth_type="u8")
    refused(ops.depth_consistency_params, CAMERA, depth_type=7)
