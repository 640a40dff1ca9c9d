"""Semi-global dense stereo on the device (ops.SgmStereoBatch: prs_sgm_stereo_batch_run) against its numpy restatement
(tests/sgm_stereo_ref.py).  Every output array is compared byte for byte over its whole allocated length: every decision of the rule
is integer arithmetic and both sides do the same three IEEE operations a pixel, so no tolerance is involved; pad columns and the
images a call must not touch are compared with the sentinel they were filled with.  A path kernel's wave owns a line (a row, or a
column start that wraps round the image) and its lanes hold 1, 2 or 4 neighbouring disparities (up to 64, 128, 256), moved as one
word when that count divides n_disparities; a winner wave takes 16 pixels; a right-winner workgroup takes 128 right pixels of a row
and stages 64 disparities at a time, 4, 2 or 1 a load as n_disparities divides; the images are worked through in chunks of
images_in_flight."""
import ctypes as C

import numpy as np
import pytest

import sgm_stereo_ref as ref
from srrg2_proslam_amd import _lib, configs, ops

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0xA5
CAM = dict(fx=40.0, fy=40.0, cx=30.0, cy=8.0, baseline_m=0.5)  # bf 20: a disparity of 4 is 5 m
DEFAULT = dict(n_disparities=16, min_disparity=0, p1=10, p2=120, n_paths=8, uniqueness_percent=10, lr_max_diff=1)


def _rng(*seed):
    return np.random.default_rng(list(seed))


def pairs(rng, shape, shift=4, noise=False):
    """left, right uint8 of `shape` = (..., rows, cols): random bytes, the left image the right one shifted by `shift` columns with a
    tenth of its pixels redrawn; noise: two unrelated images, where near-ties and the uniqueness boundary are common"""
    right = rng.integers(0, 256, shape, dtype=np.uint8)
    if noise:
        return rng.integers(0, 256, shape, dtype=np.uint8), right
    cols = shape[-1]
    left = right[..., np.clip(np.arange(cols) - shift, 0, cols - 1)].copy()
    redraw = rng.random(shape) < 0.1
    left[redraw] = rng.integers(0, 256, int(redraw.sum()), dtype=np.uint8)
    return left, right


class Rig:
    """an ops.SgmStereoBatch over device copies of left, right [B, frames, rows, cols].  pad: bytes behind every image row, random
    ones, which would change a census if they were read in the place of the clamped pixel; halves: both images in one allocation,
    the left block then the right block, as the rectifier's stereo layout has them"""

    def __init__(self, ctx, left, right, n_images=None, pad=0, outputs=ops.SgmStereoBatch.OUTPUTS, halves=False, images_in_flight=None,
                 n_disparities=256):
        import torch
        self.ctx, self.n_images, self.pad, self.halves = ctx, n_images, pad, halves
        self.B, self.frames, self.rows, self.cols = left.shape
        self.dev = torch.device("cuda", 0)
        self.ds = ops.SgmStereoBatch(self.B, self.frames, self.rows, self.cols, outputs, images_in_flight=images_in_flight,
                                     n_disparities=n_disparities)
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
            r = ref.sgm_stereo(self.left[b], self.right[b], n, rp)
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

    def run(self, cam=CAM, **kw):
        p = ops.sgm_stereo_params(cam, **dict(DEFAULT, **kw))
        self.fill_sentinel()
        self.ds.run(self.ctx, p, **self.inputs())
        self.ctx.synchronize()
        return p

    def check(self, what="", cam=CAM, **kw):
        """run and compare with the restatement; -> the restatement's results per sequence"""
        p = self.run(cam, **kw)
        want, results = self.expected(ref.params(p.bf, **dict(DEFAULT, **kw)))
        self.compare(self.outputs(), want, what)
        return results


def n_valid(results):
    return [image["n_valid"] for r in results for image in r["results"] if image is not None]


# cols: 1, 2, less than a census halo, 63, 64, 65, 130; rows: 1, 2, 3, 17, 33; (40, 7) is taller than wide: every diagonal line
# wraps more than once; 128 and 129 columns: one right-winner tile, and one pixel more
SHAPES = [(1, 1), (1, 2), (2, 1), (3, 5), (1, 65), (3, 63), (3, 64), (3, 65), (3, 130), (17, 65), (33, 65), (40, 7), (2, 128), (2, 129)]


@pytest.mark.parametrize("n_paths", [4, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes(hip_ctx, shape, n_paths):
    left, right = pairs(_rng(1, *shape), (1, 2) + shape)
    results = Rig(hip_ctx, left, right).check(n_paths=n_paths)
    assert shape[1] < 20 or min(n_valid(results)) > 0.5 * shape[0] * (shape[1] - 4)
    left, right = pairs(_rng(1, 1, *shape), (1, 1) + shape, noise=True)
    Rig(hip_ctx, left, right).check("noise", n_paths=n_paths, uniqueness_percent=3)


@pytest.mark.parametrize("min_disparity", [0, 7])
@pytest.mark.parametrize("n_disparities", [1, 2, 3, 37, 63, 64, 65, 66, 127, 128, 129, 130, 256])
def test_disparity_counts(hip_ctx, n_disparities, min_disparity):
    """the lane and register boundaries of the disparity axis: one, two and four disparities a lane, counts the lanes' word does and
    does not divide (66 and 130: two a load of the right-winner stage, one word of two a lane of the path kernel), and 1 .. 3
    disparities, which have no runner-up two away"""
    left, right = pairs(_rng(2, n_disparities, min_disparity), (1, 2, 5, 70), shift=min_disparity + min(n_disparities // 2, 20))
    rig = Rig(hip_ctx, left, right)
    rig.check(n_disparities=n_disparities, min_disparity=min_disparity)
    rig.check("4 paths, q = 0", n_disparities=n_disparities, min_disparity=min_disparity, n_paths=4, uniqueness_percent=0)


def test_256_disparities_on_40_columns_none_admissible(hip_ctx):
    left, right = pairs(_rng(3), (1, 2, 6, 40), shift=9)
    results = Rig(hip_ctx, left, right).check(n_disparities=256, min_disparity=50)
    assert max(n_valid(results)) == 0


PENALTIES = [(0, 0), (0, 5), (5, 5), (10, 120), (1, 4095), (4095, 4095)]


@pytest.mark.parametrize("penalties", PENALTIES)
def test_penalties(hip_ctx, penalties):
    left, right = pairs(_rng(4), (1, 1, 19, 45))
    if penalties == (4095, 4095):  # an 8-bit path cost cannot pass this case
        out = ref.sgm_stereo_image(left[0, 0], right[0, 0], ref.params(20.0, **dict(DEFAULT, p1=4095, p2=4095, n_paths=4)), details=True)
        assert out["max_path_cost"] > 255
    rig = Rig(hip_ctx, left, right)
    for n_paths in (4, 8):
        rig.check("%d paths" % n_paths, p1=penalties[0], p2=penalties[1], n_paths=n_paths, uniqueness_percent=0)
    rig.upload(*pairs(_rng(4, 1), (1, 1, 19, 45), noise=True))
    rig.check("noise", p1=penalties[0], p2=penalties[1])


def test_chunks_give_the_same_bytes(hip_ctx):
    left, right = pairs(_rng(5), (2, 3, 9, 67))
    first = None
    for in_flight in (1, 2, 4, 6, 100):
        rig = Rig(hip_ctx, left, right, images_in_flight=in_flight, n_disparities=16)
        assert rig.ds.images_in_flight == min(in_flight, 6)
        if first is None:
            rig.check("images_in_flight 1")
            first = rig.outputs()
        else:
            rig.run()
            rig.compare(rig.outputs(), first, "images_in_flight %d" % in_flight)


def test_images_in_flight_left_to_the_batch(hip_ctx):
    """None: at most the images of the batch; params with more disparities than the workspace was sized for are refused"""
    assert ops.SgmStereoBatch(2, 3, 9, 67).images_in_flight == 6
    sb = ops.SgmStereoBatch(1, 1, 3, 5, n_disparities=16)
    with pytest.raises(ValueError):
        sb.run(hip_ctx, ops.sgm_stereo_params(CAM, n_disparities=17), None, None)
    with pytest.raises(ValueError):
        ops.SgmStereoBatch(1, 1, 3, 5, images_in_flight=0)


def test_sequences_of_unequal_length(hip_ctx):
    left, right = pairs(_rng(8), (3, 2, 13, 61))
    rig = Rig(hip_ctx, left, right, n_images=(2, 0, 1), images_in_flight=4)
    results = rig.check()
    assert [r["status"] for r in results] == [0, 0, 0] and len(n_valid(results)) == 3


def test_a_sequence_with_too_many_images_is_refused_alone(hip_ctx):
    """three images a sequence and two in flight: the second chunk spans the refused and the served sequence"""
    left, right = pairs(_rng(9), (2, 3, 13, 61))
    for n_images in ((4, 2), (1, -1), (3, 4)):
        results = Rig(hip_ctx, left, right, n_images=n_images, images_in_flight=2).check()
        assert [r["status"] for r in results] == [ref.PRS_ERR_RANGE if not 0 <= n <= 3 else 0 for n in n_images]


@pytest.mark.parametrize("noise", [False, True])
def test_switches(hip_ctx, noise):
    left, right = pairs(_rng(5, noise), (1, 2, 19, 90), noise=noise)
    rig = Rig(hip_ctx, left, right)
    counts = {}
    for q in (0, 10):
        for lr in (-1, 0, 1):
            counts[q, lr] = sum(n_valid(rig.check("q %d lr %d" % (q, lr), uniqueness_percent=q, lr_max_diff=lr)))
    # each test only ever drops pixels
    assert counts[0, -1] >= counts[10, -1] and counts[0, -1] >= counts[0, 1] >= counts[0, 0] > 0
    assert counts[0, -1] > counts[0, 0]


@pytest.mark.parametrize("pad", [1, 29])
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
    p = ops.sgm_stereo_params(CAM, **DEFAULT)
    before = rig.outputs()
    rig.fill_sentinel()
    rig.ds.run(hip_ctx, p, whole[0].flatten(0, 1)[..., :66], whole[1].flatten(0, 1)[..., :66])
    hip_ctx.synchronize()
    rig.compare(rig.outputs(), before, "flat views")


@pytest.mark.parametrize("outputs", [("disparity",), ("depth",), ("disparity", "depth"), ("depth", "n_valid")])
def test_optional_outputs(hip_ctx, outputs):
    left, right = pairs(_rng(10), (2, 2, 9, 70))
    rig = Rig(hip_ctx, left, right, outputs=outputs)
    assert sorted(rig.tensors()) == sorted(outputs + ("status",))
    rig.check()


def test_call_level_refusals_write_nothing(hip_ctx):
    left, right = pairs(_rng(11), (2, 2, 9, 20))
    rig = Rig(hip_ctx, left, right, n_images=(2, 2))
    lib, ctx = _lib.load(), hip_ctx._h
    D = lambda: rig.ds.descriptor(**rig.inputs())  # noqa: E731
    P = lambda: ops.sgm_stereo_params(CAM, **DEFAULT)  # noqa: E731

    def run(d, p=None):
        p = P() if p is None else p
        return lib.prs_sgm_stereo_batch_run(ctx, C.byref(p) if p != "null" else None, C.byref(d) if d is not None else None)

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
                         ("out_pitch", 82), ("images_in_flight", 0), ("images_in_flight", -1)):
        d = D()
        setattr(d, field, value)
        assert run(d) == ref.PRS_ERR_RANGE, (field, value)
    for field, value in (("n_disparities", 0), ("n_disparities", 257), ("min_disparity", -1), ("min_disparity", 4081), ("n_paths", 0),
                         ("n_paths", 5), ("n_paths", 16), ("p1", -1), ("p1", 121), ("p2", 9), ("p2", 4096), ("uniqueness_percent", -1),
                         ("uniqueness_percent", 100), ("lr_max_diff", -2), ("lr_max_diff", 256), ("bf", 0.0), ("bf", -1.0), ("bf", float("nan")),
                         ("bf", float("inf"))):
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
    rig = Rig(hip_ctx, left, right, images_in_flight=4)
    rig.check("first", uniqueness_percent=2)
    first = rig.outputs()
    rig.run(uniqueness_percent=2)
    rig.compare(rig.outputs(), first, "second run")


def test_captured_graph_replayed_on_new_images(hip_ctx):
    """three chunks of two images; the replays see other images and other counts, a refused sequence among them"""
    import torch
    ctx = hip_ctx
    shape = (3, 2, 21, 75)
    rig = Rig(ctx, *pairs(_rng(13), shape), n_images=(2, 0, 1), images_in_flight=2)
    kw = dict(DEFAULT, min_disparity=1)
    p, rp = ops.sgm_stereo_params(CAM, **kw), ref.params(20.0, **kw)
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


@pytest.mark.parametrize("n_paths", [4, 8])
def test_the_textureless_wall_is_filled(hip_ctx, n_paths):
    """random texture with a flat band of 32 columns, disparity 4 everywhere: the local rule keeps none of the band's middle 288
    pixels (tests/test_sgm_stereo_ref.py), this stage all of them, within half a disparity"""
    rng = np.random.default_rng(5)
    scene = rng.integers(0, 256, (24, 100), dtype=np.uint8)
    scene[:, 34:66] = 128
    left, right = np.ascontiguousarray(scene[:, :96])[None, None], np.ascontiguousarray(scene[:, 4:])[None, None]
    rig = Rig(hip_ctx, left, right)
    rig.check(n_paths=n_paths)
    band = rig.outputs()["disparity"][0, 0, :, 42:54]
    assert int((band > 0).sum()) == 288 and (np.abs(band - 4) <= 0.5).all()


def test_real_images(hip_ctx):
    """a 128 x 512 crop of the reference's SceneFlow pair at 128 disparities, and a 96 x 400 crop of its first KITTI city pair with
    min_disparity 1 and the KITTI camera's bf"""
    import ref_pins as rp
    sf = rp.load("ref_scene_flow")
    crop = lambda image, r0, c0, rows, cols: np.ascontiguousarray(image[r0:r0 + rows, c0:c0 + cols])[None, None]  # noqa: E731
    rig = Rig(hip_ctx, crop(sf["left"], 200, 224, 128, 512), crop(sf["right"], 200, 224, 128, 512))
    results = rig.check("scene flow", n_disparities=128)
    assert n_valid(results)[0] > 0.5 * 128 * 512
    rig = Rig(hip_ctx, crop(rp.kitti_image("left", 0), 140, 420, 96, 400), crop(rp.kitti_image("right", 0), 140, 420, 96, 400))
    results = rig.check("kitti", cam=configs.KITTI["camera"], n_disparities=128, min_disparity=1)
    assert n_valid(results)[0] > 0.7 * 96 * 400
    depth = results[0]["results"][0]["depth"]
    assert 2.0 < np.median(depth[depth > 0]) < 100.0  # metres: a street


def test_stereo_filter_dense_cloud_in_place(hip_ctx):
    """SgmStereoBatch on noise pairs, the speckle filter in place on its disparity with its depth as the companion, DepthCloudBatch
    on that depth: disparity, depth and the cloud equal the same chain through the three restatements"""
    import torch

    import depth_cloud_ref as dref
    import speckle_ref as fref
    kw = dict(DEFAULT, uniqueness_percent=3)
    B, frames, rows, cols = 1, 2, 21, 70
    left, right = pairs(_rng(17), (B, frames, rows, cols), noise=True)
    stereo = ref.sgm_stereo(left[0], right[0], None, ref.params(20.0, **kw))
    disparity = np.stack([i["disparity"] for i in stereo["results"]])
    depth = np.stack([i["depth"] for i in stereo["results"]])
    filtered = fref.speckle(disparity, depth, None, fref.params(4, 1.0))
    removed = [i["n_removed"] for i in filtered["results"]]
    kept = [i["n_kept"] for i in filtered["results"]]
    assert min(removed) > 0 and min(kept) > 0  # the filter has something to remove and something to leave
    want_depth = np.stack([i["companion"] for i in filtered["results"]])

    dev = torch.device("cuda", 0)
    ds = ops.SgmStereoBatch(B, frames, rows, cols)
    ds.run(hip_ctx, ops.sgm_stereo_params(CAM, **kw), torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev))
    assert ds.depth.stride(2) == 72 and ds.depth.data_ptr() == ds._depth.data_ptr()
    sf = ops.SpeckleFilterBatch(B, frames, rows, cols)
    sf.run(hip_ctx, ops.speckle_params(4, 1.0), ds.disparity, ds.depth)
    pose = np.zeros((frames, 4, 4), F)
    for i in range(frames):
        q, _ = np.linalg.qr(_rng(17, i).normal(size=(3, 3)))
        pose[i, :3, :3], pose[i, :3, 3], pose[i, 3, 3] = q * np.sign(np.linalg.det(q)), (i, -1.0, 0.5), 1
    pose = pose.reshape(1, frames, 16)
    dc = ops.DepthCloudBatch(B, frames, rows, cols, frames * rows * cols)
    ckw = dict(range_min=0.1, range_max=10.0, scale=1.0)
    n_images = torch.tensor([frames], dtype=torch.int32, device=dev)
    dc.run(hip_ctx, ops.depth_cloud_params(CAM, depth_type="f32", **ckw), ds.depth, torch.from_numpy(pose).to(dev), n_images)
    hip_ctx.synchronize()
    assert sf.status.cpu().tolist() == [0] and sf.n_removed.cpu().tolist() == [removed] and sf.n_kept.cpu().tolist() == [kept]
    assert ds.disparity.cpu().numpy().tobytes() == np.stack([i["image"] for i in filtered["results"]])[None].tobytes()
    assert ds.depth.cpu().numpy().tobytes() == want_depth[None].tobytes()
    want = dref.depth_cloud(dict(depth=want_depth, n_images=frames, pose=pose[0]), dref.params(CAM, **ckw), dc.out_stride)
    got = dc.cloud_of(0)
    n = want["n_out"]
    assert (got["status"], got["n_out"], got["n_total"]) == (0, n, want["n_total"]) and n > 0
    assert got["xyz"].tobytes() == want["xyz"][:n].tobytes() and got["row"].tobytes() == want["pixel"][:n].tobytes()
