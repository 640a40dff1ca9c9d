"""Dense stereo on the device (ops.DenseStereoBatch: prs_dense_stereo_batch_run) against its numpy restatement
(tests/dense_stereo_ref.py).  Every output array is compared byte for byte over its whole allocated length: every decision of the
rule is integer arithmetic and both sides do the same three IEEE operations a pixel, so no tolerance is involved; pad columns and the
images a call must not touch are compared with the sentinel they were filled with.  The match kernel's workgroup owns 64 - 2 r output
columns (TILE(r)) of a band of BAND rows; the census kernel a 64 x 16 tile; the finish kernel 8 rows of an image."""
import ctypes as C

import numpy as np
import pytest

import dense_stereo_ref as ref
from srrg2_proslam_amd import _lib, configs, ops

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0xA5
BAND = 32
TILE = lambda r: 64 - 2 * r  # noqa: E731
CAM = dict(fx=40.0, fy=40.0, cx=30.0, cy=8.0, baseline_m=0.5)  # bf 20: a disparity of 4 is 5 m
DEFAULT = dict(n_disparities=16, min_disparity=0, aggregation_radius=3, uniqueness_percent=10, lr_max_diff=1)


def _rng(*seed):
    return np.random.default_rng(list(seed))


def pairs(rng, shape, shift=4, noise=False):
    """left, right uint8 of `shape` = (..., rows, cols): random bytes, the left image the right one shifted by `shift` columns with a
    tenth of its pixels redrawn, so winners are not all ties and some pixels fail a test; noise: two unrelated images, where
    near-ties and the uniqueness boundary are common"""
    right = rng.integers(0, 256, shape, dtype=np.uint8)
    if noise:
        return rng.integers(0, 256, shape, dtype=np.uint8), right
    cols = shape[-1]
    left = right[..., np.clip(np.arange(cols) - shift, 0, cols - 1)].copy()
    redraw = rng.random(shape) < 0.1
    left[redraw] = rng.integers(0, 256, int(redraw.sum()), dtype=np.uint8)
    return left, right


class Rig:
    """an ops.DenseStereoBatch over device copies of left, right [B, frames, rows, cols].  pad: bytes behind every image row, random
    ones, which would change a census if they were read in the place of the clamped pixel; halves: both images in one allocation,
    the left block then the right block, as the rectifier's stereo layout has them"""

    def __init__(self, ctx, left, right, n_images=None, pad=0, outputs=ops.DenseStereoBatch.OUTPUTS, halves=False):
        import torch
        self.ctx, self.n_images, self.pad, self.halves = ctx, n_images, pad, halves
        self.B, self.frames, self.rows, self.cols = left.shape
        self.dev = torch.device("cuda", 0)
        self.ds = ops.DenseStereoBatch(self.B, self.frames, self.rows, self.cols, outputs)
        self.images = torch.zeros((2,) + left.shape[:3] + (self.cols + pad,), dtype=torch.uint8, device=self.dev)
        if not halves:
            self.images = [self.images[0].clone(), self.images[1].clone()]
        self.t_n = torch.zeros((self.B,), dtype=torch.int32, device=self.dev) if n_images is not None else None
        self.upload(left, right, n_images)

    def upload(self, left, right, n_images=None):
        import torch
        self.left, self.right, self.n_images = left, right, n_images
        for i, host in enumerate((left, right)):
            full = _rng(99, i, self.cols).integers(0, 256, host.shape[:3] + (self.cols + self.pad,), dtype=np.uint8)
            full[..., :self.cols] = host
            self.images[i].copy_(torch.from_numpy(full))
        if n_images is not None:
            self.t_n.copy_(torch.tensor(n_images, dtype=torch.int32))

    def inputs(self):
        return dict(left=self.images[0][..., :self.cols], right=self.images[1][..., :self.cols], n_images=self.t_n)

    def tensors(self):
        out = dict(disparity=self.ds._disparity, depth=self.ds._depth, n_valid=self.ds.n_valid, status=self.ds.status)
        return {k: t for k, t in out.items() if t is not None}

    def fill_sentinel(self):
        import torch
        for t in self.tensors().values():
            t.view(torch.uint8).fill_(SENTINEL)

    def outputs(self):
        return {k: t.cpu().numpy() for k, t in self.tensors().items()}

    def expected(self, rp):
        """every output array as the call must leave a sentinel-filled one, and the restatement's results per sequence"""
        want = {k: np.full(tuple(t.shape), SENTINEL, np.uint8).repeat(4, axis=-1).view(F if k in ("disparity", "depth") else np.int32)
                for k, t in self.tensors().items()}
        results = []
        for b in range(self.B):
            n = None if self.n_images is None else self.n_images[b]
            r = ref.dense_stereo(self.left[b], self.right[b], n, rp)
            results.append(r)
            want["status"][b] = r["status"]
            for f, image in enumerate(r["results"]):
                if image is not None:
                    for k in ("disparity", "depth"):
                        if k in want:
                            want[k][b, f, :, :self.cols] = image[k]
                    if "n_valid" in want:
                        want["n_valid"][b, f] = image["n_valid"]
        return want, results

    def compare(self, got, want, what=""):
        for k in want:
            assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k, np.argwhere(got[k] != want[k])[:5])

    def check(self, what="", cam=CAM, **kw):
        """run and compare with the restatement; -> the restatement's results per sequence"""
        kw = dict(DEFAULT, **kw)
        p = ops.dense_stereo_params(cam, **kw)
        self.fill_sentinel()
        self.ds.run(self.ctx, p, **self.inputs())
        self.ctx.synchronize()
        want, results = self.expected(ref.params(p.bf, **kw))
        self.compare(self.outputs(), want, what)
        return results


def n_valid(results):
    return [image["n_valid"] for r in results for image in r["results"] if image is not None]


# cols: 1, less than a census halo, TILE(3) - 1, TILE(3), TILE(3) + 1, 63, 64, 65, three tiles; rows: 1, 3, 17 (two census tiles),
# BAND + 1 (two bands)
SHAPES = [(1, 1), (3, 1), (3, 5), (3, 57), (3, 58), (3, 59), (3, 63), (3, 64), (3, 65), (3, 130), (1, 65), (17, 65), (BAND + 1, 65)]


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes(hip_ctx, shape):
    left, right = pairs(_rng(1, *shape), (2, 2) + shape)
    results = Rig(hip_ctx, left, right).check()
    assert shape[1] < 20 or min(n_valid(results)) > 0.5 * shape[0] * (shape[1] - 4)
    # the tile's edges move with the radius: TILE(1) = 62, TILE(0) = 64
    left, right = pairs(_rng(1, 1, *shape), (1, 1) + shape, noise=True)
    rig = Rig(hip_ctx, left, right)
    for r in (0, 1):
        rig.check("noise, r = %d" % r, aggregation_radius=r, uniqueness_percent=3)


@pytest.mark.parametrize("min_disparity", [0, 1, 7])
@pytest.mark.parametrize("n_disparities", [1, 2, 3, 16, 37])
def test_disparity_ranges(hip_ctx, n_disparities, min_disparity):
    """1 .. 3 disparities have no runner-up two away; 37 fills neither a word pair nor the four waves' turns evenly"""
    left, right = pairs(_rng(2, n_disparities, min_disparity), (2, 1, 17, 70), shift=min_disparity + n_disparities // 2)
    rig = Rig(hip_ctx, left, right)
    results = rig.check(n_disparities=n_disparities, min_disparity=min_disparity, aggregation_radius=1)
    assert min_disparity + n_disparities // 2 == 0 or min(n_valid(results)) > 300
    rig.check("q = 0", n_disparities=n_disparities, min_disparity=min_disparity, aggregation_radius=1, uniqueness_percent=0)


@pytest.mark.parametrize("min_disparity", [0, 7, 50])
def test_256_disparities_on_40_columns(hip_ctx, min_disparity):
    """most disparities are inadmissible, and pixels with u < min_disparity (all of them at 50) have none"""
    left, right = pairs(_rng(3, min_disparity), (1, 2, 6, 40), shift=9)
    results = Rig(hip_ctx, left, right).check(n_disparities=256, min_disparity=min_disparity, aggregation_radius=1)
    assert (min(n_valid(results)) > 100) == (min_disparity < 50) and (max(n_valid(results)) == 0) == (min_disparity == 50)


@pytest.mark.parametrize("rows,r", [(17, 0), (17, 1), (17, 3), (5, 7), (BAND + 3, 7)])
def test_radius(hip_ctx, rows, r):
    """r = 7 on 5 rows: the window is taller than the image; on BAND + 3 rows the second band starts inside the first one's window"""
    left, right = pairs(_rng(4, rows, r), (1, 2, rows, 70))
    rig = Rig(hip_ctx, left, right)
    assert min(n_valid(rig.check(aggregation_radius=r))) > 0.5 * rows * 66
    noise = pairs(_rng(4, rows, r, 1), (1, 2, rows, 70), noise=True)
    rig.upload(*noise)
    rig.check("noise", aggregation_radius=r, uniqueness_percent=1)


@pytest.mark.parametrize("noise", [False, True])
def test_switches(hip_ctx, noise):
    left, right = pairs(_rng(5, noise), (1, 2, 19, 90), noise=noise)
    rig = Rig(hip_ctx, left, right)
    counts = {}
    for q in (0, 10, 99):
        for lr in (-1, 0, 1):
            counts[q, lr] = sum(n_valid(rig.check("q %d lr %d" % (q, lr), uniqueness_percent=q, lr_max_diff=lr, aggregation_radius=1)))
    # each test only ever drops pixels
    assert counts[0, -1] >= counts[10, -1] >= counts[99, -1] and counts[0, -1] >= counts[0, 1] >= counts[0, 0] > 0
    assert counts[0, -1] > counts[99, -1] and counts[0, -1] > counts[0, 0]


@pytest.mark.parametrize("pad", [1, 4, 29])
def test_an_input_pitch_with_padding(hip_ctx, pad):
    left, right = pairs(_rng(6, pad), (2, 2, 9, 67))
    rig = Rig(hip_ctx, left, right, pad=pad)
    assert rig.inputs()["left"].stride(2) == 67 + pad
    rig.check()


def test_left_and_right_as_halves_of_one_allocation(hip_ctx):
    """the rectifier's stereo layout: [2 * B * frames, rows, pitch], the left block then the right block, passed as its two halves"""
    left, right = pairs(_rng(7), (2, 3, 11, 66))
    rig = Rig(hip_ctx, left, right, pad=2, halves=True)
    whole = rig.images
    assert rig.inputs()["right"].data_ptr() == whole.data_ptr() + 2 * 3 * 11 * 68
    rig.check()
    # and as the flat [B * frames, rows, cols] views RectifyBatch.left / .right are
    p = ops.dense_stereo_params(CAM, **DEFAULT)
    before = rig.outputs()
    rig.fill_sentinel()
    rig.ds.run(hip_ctx, p, whole[0].flatten(0, 1)[..., :66], whole[1].flatten(0, 1)[..., :66])
    hip_ctx.synchronize()
    rig.compare(rig.outputs(), before, "flat views")


def test_sequences_of_unequal_length(hip_ctx):
    left, right = pairs(_rng(8), (3, 2, 13, 61))
    rig = Rig(hip_ctx, left, right, n_images=(2, 0, 1))
    results = rig.check()
    assert [r["status"] for r in results] == [0, 0, 0] and len(n_valid(results)) == 3


def test_a_sequence_with_too_many_images_is_refused_alone(hip_ctx):
    left, right = pairs(_rng(9), (2, 2, 13, 61))
    for n_images in ((3, 2), (1, -1)):
        results = Rig(hip_ctx, left, right, n_images=n_images).check()
        assert [r["status"] for r in results] == [ref.PRS_ERR_RANGE if not 0 <= n <= 2 else 0 for n in n_images]


@pytest.mark.parametrize("outputs", [("disparity",), ("depth",), ("disparity", "depth"), ("depth", "n_valid")])
def test_optional_outputs(hip_ctx, outputs):
    """disparity only, depth only, and neither n_valid nor n_images"""
    left, right = pairs(_rng(10), (2, 2, 9, 70))
    rig = Rig(hip_ctx, left, right, outputs=outputs)
    assert sorted(rig.tensors()) == sorted(outputs + ("status",))
    rig.check()


def test_call_level_refusals_write_nothing(hip_ctx):
    left, right = pairs(_rng(11), (2, 2, 9, 20))
    rig = Rig(hip_ctx, left, right, n_images=(2, 2))
    lib, ctx = _lib.load(), hip_ctx._h
    D = lambda: rig.ds.descriptor(**rig.inputs())  # noqa: E731
    P = lambda: ops.dense_stereo_params(CAM, **DEFAULT)  # noqa: E731

    def run(d, p=None):
        p = P() if p is None else p
        return lib.prs_dense_stereo_batch_run(ctx, C.byref(p) if p != "null" else None, C.byref(d) if d is not None else None)

    rig.fill_sentinel()
    assert run(D()) == 0
    hip_ctx.synchronize()
    rig.fill_sentinel()
    assert run(None) == -1 and run(D(), "null") == -1
    for field in ("left", "right", "status", "workspace"):
        d = D()
        setattr(d, field, None)
        assert run(d) == -1, field
    d = D()
    d.disparity, d.depth = None, None
    assert run(d) == -1
    for field, value in (("batch", 0), ("frames", 0), ("rows", 0), ("cols", -1), ("left_pitch", 19), ("right_pitch", 19), ("out_pitch", 76),
                         ("out_pitch", 82)):
        d = D()
        setattr(d, field, value)
        assert run(d) == ref.PRS_ERR_RANGE, (field, value)
    for field, value in (("n_disparities", 0), ("n_disparities", 257), ("min_disparity", -1), ("min_disparity", 4081), ("aggregation_radius", -1),
                         ("aggregation_radius", 8), ("uniqueness_percent", -1), ("uniqueness_percent", 100), ("lr_max_diff", -2),
                         ("lr_max_diff", 256), ("bf", 0.0), ("bf", -1.0), ("bf", float("nan")), ("bf", float("inf"))):
        p = P()
        setattr(p, field, value)
        assert run(D(), p) == ref.PRS_ERR_RANGE, (field, value)
    for field, step in (("disparity", 2), ("depth", 1), ("workspace", 8), ("n_images", 2), ("n_valid", 1), ("status", 2)):
        d = D()
        setattr(d, field, getattr(d, field) + step)
        assert run(d) == -5, field
    # 2^16 x 2^15 pixels are too many for an image, 2^12 images of 2^10 x 2^10 too many for a call
    for rows, cols, frames in ((1 << 16, 1 << 15, 2), (1 << 10, 1 << 10, 1 << 12)):
        d = D()
        d.rows, d.cols, d.frames, d.left_pitch, d.right_pitch, d.out_pitch = rows, cols, frames, cols, cols, 4 * cols
        assert run(d) == -5, (rows, cols, frames)
    hip_ctx.synchronize()
    for k, v in rig.outputs().items():
        assert (v.view(np.uint8) == SENTINEL).all(), k


def test_two_runs_are_byte_identical(hip_ctx):
    left, right = pairs(_rng(12), (3, 2, 37, 131), noise=True)
    rig = Rig(hip_ctx, left, right)
    rig.check("first", uniqueness_percent=2)
    first = rig.outputs()
    rig.check("second", uniqueness_percent=2)
    rig.compare(rig.outputs(), first, "second run")


def test_captured_graph_replayed_on_new_images(hip_ctx):
    import torch
    ctx = hip_ctx
    shape = (3, 2, 21, 75)
    rig = Rig(ctx, *pairs(_rng(13), shape), n_images=(2, 0, 1))
    kw = dict(DEFAULT, min_disparity=1)
    p, rp = ops.dense_stereo_params(CAM, **kw), ref.params(20.0, **kw)
    inputs = rig.inputs()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        rig.ds.run(ctx, p, **inputs)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rig.ds.run(ctx, p, **inputs)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    torch.cuda.synchronize()
    # other images and counts, a refused sequence among them
    for replay, counts in enumerate(((1, 2, 2), (0, 3, 2))):
        left, right = pairs(_rng(13, replay), shape, shift=3 + replay, noise=replay == 1)
        rig.upload(left, right, counts)
        rig.fill_sentinel()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want, results = rig.expected(rp)
        rig.compare(rig.outputs(), want, "replay %d" % replay)
        assert [r["status"] for r in results] == ([0, 0, 0] if replay == 0 else [0, ref.PRS_ERR_RANGE, 0])


def test_real_images(hip_ctx):
    """a 128 x 512 crop of the reference's SceneFlow pair at 128 disparities, and a 96 x 400 crop of its first KITTI city pair with
    min_disparity 1 and the KITTI camera's bf"""
    import ref_pins as rp
    sf = rp.load("ref_scene_flow")
    crop = lambda image, r0, c0, rows, cols: np.ascontiguousarray(image[r0:r0 + rows, c0:c0 + cols])[None, None]  # noqa: E731
    rig = Rig(hip_ctx, crop(sf["left"], 200, 224, 128, 512), crop(sf["right"], 200, 224, 128, 512))
    results = rig.check("scene flow", n_disparities=128)
    assert n_valid(results)[0] > 0.2 * 128 * 512
    rig = Rig(hip_ctx, crop(rp.kitti_image("left", 0), 140, 420, 96, 400), crop(rp.kitti_image("right", 0), 140, 420, 96, 400))
    results = rig.check("kitti", cam=configs.KITTI["camera"], n_disparities=128, min_disparity=1)
    assert n_valid(results)[0] > 0.2 * 96 * 400
    depth = results[0]["results"][0]["depth"]
    assert 2.0 < np.median(depth[depth > 0]) < 100.0  # metres: a street


def test_depth_goes_into_the_dense_cloud_in_place(hip_ctx):
    """DenseStereoBatch.depth of two small frames, with two poses, into DepthCloudBatch.run as float32 depth at scale 1: the cloud
    equals the dense cloud's restatement applied to this stage's restatement"""
    import torch

    import depth_cloud_ref as dref
    rows, cols, frames = 21, 70, 2
    left, right = pairs(_rng(14), (1, frames, rows, cols))
    rig = Rig(hip_ctx, left, right)
    results = rig.check(aggregation_radius=2)
    pose = np.zeros((frames, 4, 4), F)
    for i in range(frames):
        q, _ = np.linalg.qr(_rng(14, i).normal(size=(3, 3)))
        pose[i, :3, :3], pose[i, :3, 3], pose[i, 3, 3] = q * np.sign(np.linalg.det(q)), (i, -1.0, 0.5), 1
    pose = pose.reshape(1, frames, 16)
    depth = rig.ds.depth
    assert depth.stride(2) == 72 and depth.data_ptr() == rig.ds._depth.data_ptr()
    dc = ops.DepthCloudBatch(1, frames, rows, cols, frames * rows * cols)
    kw = dict(range_min=0.1, range_max=10.0, scale=1.0)
    n_images = torch.tensor([frames], dtype=torch.int32, device="cuda")
    dc.run(hip_ctx, ops.depth_cloud_params(CAM, depth_type="f32", **kw), depth, torch.from_numpy(pose).to("cuda"), n_images)
    hip_ctx.synchronize()
    want_depth = np.stack([image["depth"] for image in results[0]["results"]])
    want = dref.depth_cloud(dict(depth=want_depth, n_images=frames, pose=pose[0]), dref.params(CAM, **kw), dc.out_stride)
    got = dc.cloud_of(0)
    n = want["n_out"]
    assert (got["status"], got["n_out"], got["n_total"]) == (0, n, want["n_total"]) and n > 0.5 * frames * rows * cols
    assert got["xyz"].tobytes() == want["xyz"][:n].tobytes() and got["node"].tobytes() == want["frame"][:n].tobytes()
    assert got["row"].tobytes() == want["pixel"][:n].tobytes()
