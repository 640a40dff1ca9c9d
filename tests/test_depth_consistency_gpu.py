"""The depth consistency filter on the device (ops.DepthConsistencyBatch: prs_depth_consistency_batch_run) against its numpy
restatement (tests/depth_consistency_ref.py).  Every output array is compared byte for byte over its whole allocated length: every
operation of the rule is stated, so no tolerance is involved; pad columns, the images a call must not touch and the outputs of a
refused sequence are compared with the sentinel they were filled with.  A filter workgroup owns TW x TH pixels of one image and
works through them in steps of TW x STEP."""
import ctypes as C

import numpy as np
import pytest

import depth_consistency_ref as ref
import test_depth_consistency_ref as cases
from srrg2_proslam_amd import _lib, ops

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0xA5
TW, TH, STEP = 64, 32, 4
TORCH = {np.dtype(np.float32): "float32", np.dtype(np.uint16): "uint16"}
TYPE = {np.dtype(np.float32): "f32", np.dtype(np.uint16): "u16"}
OUTPUTS = ops.DepthConsistencyBatch.OUTPUTS


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


def sentinel(shape, dtype):
    dtype = np.dtype(dtype)
    return np.full(tuple(shape) + (dtype.itemsize,), SENTINEL, np.uint8).view(dtype).reshape(tuple(shape))


class Rig:
    """an ops.DepthConsistencyBatch over device copies of depth [B, frames, rows, cols] (float32 or uint16) and pose [B, poses, 16].
    pad: elements behind every row of depth, holding a valid depth that would vote if it were read"""

    def __init__(self, ctx, depth, pose, n_images=None, frame_index=None, pad=0, window=8, outputs=OUTPUTS):
        import torch
        self.ctx, self.pad = ctx, pad
        self.B, self.frames, self.rows, self.cols = depth.shape
        self.dev = torch.device("cuda", 0)
        self.dcb = ops.DepthConsistencyBatch(self.B, self.frames, self.rows, self.cols, window, TYPE[depth.dtype], outputs)
        self.t_depth = torch.zeros(depth.shape[:3] + (self.cols + pad,), dtype=getattr(torch, TORCH[depth.dtype]), device=self.dev)
        self.t_pose = torch.zeros(pose.shape, dtype=torch.float32, device=self.dev)
        self.t_n = torch.zeros((self.B,), dtype=torch.int32, device=self.dev) if n_images is not None else None
        self.t_index = torch.zeros((self.B, self.frames), dtype=torch.int32, device=self.dev) if frame_index is not None else None
        self.upload(depth, pose, n_images, frame_index)

    def upload(self, depth, pose, n_images=None, frame_index=None):
        import torch
        self.depth, self.pose, self.n_images, self.frame_index = depth, np.asarray(pose, F), n_images, frame_index
        full = depth if self.pad == 0 else np.concatenate([depth, np.full(depth.shape[:3] + (self.pad,), 4 if depth.dtype == F else 4000, depth.dtype)], -1)
        self.t_depth.copy_(torch.from_numpy(np.ascontiguousarray(full)))
        self.t_pose.copy_(torch.from_numpy(self.pose))
        if n_images is not None:
            self.t_n.copy_(torch.tensor(n_images, dtype=torch.int32))
        if frame_index is not None:
            self.t_index.copy_(torch.from_numpy(np.asarray(frame_index, np.int32)))

    def inputs(self):
        return dict(depth=self.t_depth[..., :self.cols], pose=self.t_pose, n_images=self.t_n, frame_index=self.t_index)

    def tensors(self):
        d = self.dcb
        out = dict(out=d._out, support=d._support, violation=d._violation, n_kept=d.n_kept, n_removed=d.n_removed, n_skipped=d.n_skipped,
                   status=d.status)
        return {k: t for k, t in out.items() if t is not None}

    def fill_sentinel(self):
        import torch
        for t in self.tensors().values():
            t.view(torch.uint8).fill_(SENTINEL)

    def outputs(self):
        return {k: t.cpu().numpy() for k, t in self.tensors().items()}

    def expected(self, rp):
        """every array as the call must leave it from a sentinel-filled state, and the restatement's results per sequence"""
        want = {k: sentinel(t.shape, self.depth.dtype if k == "out" else np.uint8 if k in ("support", "violation") else np.int32)
                for k, t in self.tensors().items()}
        results = []
        for b in range(self.B):
            seq = dict(depth=self.depth[b], pose=self.pose[b], n_images=None if self.n_images is None else self.n_images[b],
                       frame_index=None if self.frame_index is None else self.frame_index[b])
            r = ref.depth_consistency(seq, rp)
            results.append(r)
            want["status"][b] = r["status"]
            if "n_skipped" in want:
                want["n_skipped"][b] = r["n_skipped"]
            for f, image in enumerate(r["results"]):
                if image is not None:
                    for k in ("out", "support", "violation"):
                        if k in want:
                            want[k][b, f, :, :self.cols] = image[k]
                    for k in ("n_kept", "n_removed"):
                        if k in want:
                            want[k][b, f] = image[k]
        return want, results

    def compare(self, got, want, what=""):
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
            assert got[k].tobytes() == want[k].tobytes(), (what, k, np.argwhere(got[k] != want[k])[:5])

    def check(self, camera, what="", **kw):
        """run and compare with the restatement; -> its results per sequence"""
        scale = kw.pop("scale", 1.0 if self.depth.dtype == F else 1e-3)
        p = ops.depth_consistency_params(camera, depth_type=TYPE[self.depth.dtype], scale=scale, **kw)
        self.fill_sentinel()
        out = self.dcb.run(self.ctx, p, **self.inputs())
        assert out.data_ptr() == self.dcb._out.data_ptr() and tuple(out.shape) == self.depth.shape
        self.ctx.synchronize()
        want, results = self.expected(ref.params(camera, scale=scale, **kw))
        self.compare(self.outputs(), want, (what, kw))
        return results


def images_of(results):
    return [image for r in results for image in r["results"] if image is not None]


def camera_of(rows, cols):
    f = 0.9 * max(rows, cols)
    return dict(fx=f, fy=f + 0.5, cx=(cols - 1) / 2 + 0.25, cy=(rows - 1) / 2)


def sequences(rng, B, frames, rows, cols, dtype, origin=(0.0, 0.0, 0.0), poses=None):
    """(depth [B, frames, rows, cols], pose [B, poses, 16], camera): cameras a few centimetres and milliradians apart in front of a
    wall 4 m away, whose depth carries 0.5 % of noise; a tenth of the pixels hold a depth off by a factor, a tenth no depth, and a
    float image a few values that are none.  All three votes and the occlusion occur"""
    camera = camera_of(rows, cols)
    poses = frames if poses is None else poses
    pose = np.zeros((B, poses, 16), F)
    for b in range(B):
        for i in range(poses):
            T = ref.yaw_pose(rng.normal(0, 0.004), np.asarray(origin) + rng.normal(0, 0.03, 3)).reshape(4, 4)
            T[3] = (7, 8, 9, 10)  # the bottom row is never read
            pose[b, i] = T.reshape(16)
    z = pose.reshape(B, poses, 4, 4)[:, :frames, 2, 3] - F(origin[2]) if poses >= frames else np.zeros((B, frames), F)
    shape = (B, frames, rows, cols)
    depth = (4.0 - z[..., None, None]) * (1 + rng.normal(0, 0.005, shape))
    off = rng.random(shape) < 0.1
    depth = np.where(off, depth * np.where(rng.random(shape) < 0.5, rng.uniform(0.5, 0.9, shape), rng.uniform(1.1, 2.0, shape)), depth)
    depth[rng.random(shape) < 0.1] = 0
    depth[rng.random(shape) < 0.02] = 12  # beyond range_max
    if dtype == np.uint16:
        return np.round(depth * 1000).astype(np.uint16), pose, camera
    depth = depth.astype(F)
    odd = rng.random(shape)
    for lo, value in ((0.00, np.nan), (0.01, np.inf), (0.02, -np.inf), (0.03, -0.0), (0.04, -4.0)):
        depth[(odd >= lo) & (odd < lo + 0.01)] = value
    return depth, pose, camera


# ---- 1. tile geometry ----------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 2), (5, 65), (48, 64), (7, 130), (STEP, TW), (TH, TW), (TH + 1, TW - 1), (2 * TH + STEP + 1, TW + 1)]


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes(hip_ctx, shape, dtype):
    """tile edges in both directions; the pad columns of out, support and violation keep their sentinel, those of depth are not read"""
    depth, pose, camera = sequences(_rng(1, *shape), 2, 3, *shape, dtype)
    rig = Rig(hip_ctx, depth, pose, pad=3)
    assert rig.dcb._out.shape[3] == (shape[1] + 3) // 4 * 4 and rig.inputs()["depth"].stride(2) == shape[1] + 3
    results = rig.check(camera, window=2, min_support=1)
    images = images_of(results)
    if shape[0] * shape[1] > 100:
        assert all(i["n_kept"] > 0 and i["n_removed"] > 0 for i in images)
        assert sum(int(i["violation"].sum()) for i in images) > 0 and max(int(i["support"].max()) for i in images) == 2
    rig.check(camera, window=1, min_support=0, max_violation=0)


# ---- 2. neighbours -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [1, 2, 5, 17])
@pytest.mark.parametrize("window,stride", [(1, 1), (2, 1), (8, 1), (1, 3), (2, 3), (8, 3)])
def test_windows_and_strides(hip_ctx, frames, window, stride):
    depth, pose, camera = sequences(_rng(2, frames), 1, frames, TH + 3, TW + 6, np.uint16)
    rig = Rig(hip_ctx, depth, pose)
    results = rig.check(camera, window=window, stride=stride, min_support=1, max_violation=2)
    slots = [sum(0 <= g < frames for g in ref.slots_of(f, dict(window=window, stride=stride))) for f in range(frames)]
    for f, image in enumerate(images_of(results)):
        assert int(image["support"].max()) <= slots[f] and (slots[f] > 0) == (image["n_kept"] > 0)
    if frames == 17 and stride == 1:
        assert max(int(i["support"].max()) for i in images_of(results)) > min(window, 4)


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_n_images_below_frames_leaves_the_tail(hip_ctx, dtype):
    depth, pose, camera = sequences(_rng(3), 3, 4, 6, 70, dtype)
    rig = Rig(hip_ctx, depth, pose, n_images=(2, 0, 4))
    results = rig.check(camera, window=2, min_support=1)
    assert [sum(i is not None for i in r["results"]) for r in results] == [2, 0, 4]
    out = rig.outputs()
    assert (out["out"][0, 2:].view(np.uint8) == SENTINEL).all() and (out["n_kept"][1].view(np.uint8) == SENTINEL).all()
    assert out["status"].tolist() == [0, 0, 0] and out["n_skipped"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_a_batch_with_a_refused_sequence(hip_ctx, dtype):
    """three sequences with poses of their own and a sensor off the robot's origin; the second's n_images is out of range: its status
    says so, n_skipped is 0, and nothing else of it is written; the others are as if they were alone"""
    depth, pose, camera = sequences(_rng(4), 3, 5, 9, 67, dtype)
    S = ref.yaw_pose(0.3, (0.1, -0.2, 0.3))
    for bad in (6, -1):
        rig = Rig(hip_ctx, depth, pose, n_images=(5, bad, 3))
        results = rig.check(camera, window=2, min_support=1, sensor_in_robot=S)
        out = rig.outputs()
        assert out["status"].tolist() == [0, ref.PRS_ERR_RANGE, 0] and out["n_skipped"].tolist() == [0, 0, 0]
        for k in ("out", "support", "violation", "n_kept", "n_removed"):
            assert (out[k][1].view(np.uint8) == SENTINEL).all(), k
        alone = ref.depth_consistency(dict(depth=depth[2], pose=pose[2], n_images=3), ref.params(camera, min_support=1, sensor_in_robot=S,
                                                                                                 scale=1.0 if dtype == np.float32 else 1e-3))
        assert all(results[2]["results"][f]["out"].tobytes() == alone["results"][f]["out"].tobytes() for f in range(3))


def test_frame_index_with_an_entry_out_of_range_and_a_nan_pose(hip_ctx):
    depth, pose, camera = sequences(_rng(5), 2, 6, 7, 66, np.float32, poses=9)
    pose[0, 4, 6] = np.nan
    pose[1, 2, 11] = np.inf
    pose[1, 0, 13] = np.nan  # the bottom row: still usable
    index = np.array([[8, 4, 0, 9, 2, -1], [0, 1, 2, 3, 4, 5]], np.int32)
    rig = Rig(hip_ctx, depth, pose, frame_index=index)
    results = rig.check(camera, window=2, min_support=1)
    assert [r["n_skipped"] for r in results] == [3, 1]
    skipped = results[0]["results"][1]
    assert not skipped["out"].any() and skipped["n_kept"] == 0 and skipped["n_removed"] > 0
    assert results[0]["results"][0]["n_kept"] > 0  # its neighbour two frames on is usable
    # without n_removed the skipped frames' depth is not needed; the other outputs are the same
    rig = Rig(hip_ctx, depth, pose, frame_index=index, outputs=("support", "n_kept", "n_skipped"))
    rig.check(camera, window=2, min_support=1)


def test_far_from_the_origin(hip_ctx):
    """poses a kilometre out: the relative transform is formed in float64, as the restatement forms it"""
    depth, pose, camera = sequences(_rng(6), 1, 5, 9, 70, np.float32, origin=(600.0, 800.0, -20.0))
    results = Rig(hip_ctx, depth, pose).check(camera, window=2)
    assert all(i["n_kept"] > 0.3 * i["out"].size for i in images_of(results))


@pytest.mark.parametrize("outputs", [(), ("support",), ("violation", "n_removed"), ("n_kept",), ("n_skipped",)])
def test_optional_outputs(hip_ctx, outputs):
    depth, pose, camera = sequences(_rng(7), 2, 3, TH + 1, TW + 2, np.uint16)
    pose[1, 1, 0] = np.nan
    rig = Rig(hip_ctx, depth, pose, outputs=outputs)
    assert sorted(rig.tensors()) == sorted(outputs + ("out", "status"))
    rig.check(camera, window=1, min_support=1)


def test_default_outputs():
    d = ops.DepthConsistencyBatch(1, 2, 2, 2, 2)
    assert d.support is None and d.violation is None and d.n_skipped is None and d.n_kept is not None and d.n_removed is not None
    assert d.out.dtype == d._out.dtype and str(d.out.dtype) == "torch.uint16" and d.workspace.numel() == 64 * 2 * 4


# ---- 3. the hand-made cases of the restatement's tests ---------------------------------------------------------------------------------
def test_tolerance_case(hip_ctx):
    depth, pose = cases.tolerance_case()
    r = Rig(hip_ctx, depth[None], pose[None]).check(cases.CAMERA, window=1, max_rel_diff=0.25, min_support=1, max_violation=0)
    assert r[0]["results"][0]["support"].tolist() == [[1, 1, 0, 0]] and r[0]["results"][0]["violation"].tolist() == [[0, 0, 1, 0]]


def test_border_case(hip_ctx):
    depth, pose = cases.border_case()
    r = Rig(hip_ctx, depth[None], pose[None], pad=2).check(cases.CAMERA, window=1, min_support=2)
    assert (r[0]["results"][1]["support"] == np.array([2, 2, 2, 2, 1], np.uint8)).all()


def test_neighbour_that_looks_the_other_way(hip_ctx):
    depth, pose = np.full((1, 2, 3, 3), 4, F), np.stack([cases.EYE, cases.half_turn_about_y()])[None]
    r = Rig(hip_ctx, depth, pose).check(cases.CAMERA, window=1, min_support=0, max_violation=0)
    assert not r[0]["results"][0]["support"].any()


def test_odd_values_case(hip_ctx):
    depths, pose = cases.odd_values_case()
    for depth in depths:
        Rig(hip_ctx, depth[None], pose[None]).check(cases.CAMERA, window=1, min_support=1)


def test_nan_projection_case(hip_ctx):
    depth, pose = cases.nan_projection_case()
    r = Rig(hip_ctx, depth[None], pose[None]).check(cases.CAMERA, window=1, min_support=0, max_violation=0)
    assert not r[0]["results"][0]["support"].any() and (r[0]["results"][0]["out"] == 4).all()


def test_unusable_case(hip_ctx):
    depth, pose, index = cases.unusable_case()
    rig = Rig(hip_ctx, depth[None], pose[None], frame_index=index[None])
    for window in (1, 2):
        r = rig.check(cases.CAMERA, window=window, min_support=1)
        assert r[0]["n_skipped"] == 2


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_without_a_decision_out_is_the_input_where_valid(hip_ctx, dtype):
    depth, pose, camera = sequences(_rng(8), 1, 3, 9, 70, dtype)
    rig = Rig(hip_ctx, depth, pose)
    rig.check(camera, window=1, min_support=0, max_violation=16)
    out = rig.outputs()["out"][..., :70]
    ok = np.stack([ref.valid(image, ref.params(camera, scale=1.0 if dtype == np.float32 else 1e-3))[0] for image in depth[0]])[None]
    assert out[ok].tobytes() == depth[ok].tobytes() and not out[~ok].view(np.uint8).any() and 0 < ok.sum() < ok.size


# ---- 4. the synthetic scene ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return ref.scene()


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_scene(hip_ctx, scene, dtype):
    seq, planted = scene
    depth = seq["depth"] if dtype == np.float32 else np.round(seq["depth"] * 1000).astype(np.uint16)
    results = Rig(hip_ctx, depth[None], seq["pose"][None]).check(ref.SCENE_CAMERA, **{k: v for k, v in ref_defaults().items()})
    kept = np.stack([i["out"] > 0 for i in images_of(results)])
    assert kept[planted].mean() <= 0.02 and kept[2][~planted[2]].mean() >= 0.85


def ref_defaults():
    from srrg2_proslam_amd import configs
    return dict(configs.DEPTH_CONSISTENCY)


# ---- 5. determinism and capture ------------------------------------------------------------------------------------------------------
def test_captured_graph_replayed_twice(hip_ctx):
    import torch
    ctx = hip_ctx
    depth, pose, camera = sequences(_rng(9), 2, 5, 2 * TH + 1, TW + 9, np.float32)
    rig = Rig(ctx, depth, pose, n_images=(5, 4))
    kw = dict(window=2, min_support=1)
    rig.check(camera, **kw)
    eager = rig.outputs()
    p = ops.depth_consistency_params(camera, depth_type="f32", **kw)
    inputs = rig.inputs()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        rig.dcb.run(ctx, p, **inputs)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rig.dcb.run(ctx, p, **inputs)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    torch.cuda.synchronize()
    for replay in range(2):
        rig.fill_sentinel()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        rig.compare(rig.outputs(), eager, "replay %d" % replay)
    # and on other images
    depth2, pose2, _ = sequences(_rng(9, 1), 2, 5, 2 * TH + 1, TW + 9, np.float32)
    rig.upload(depth2, pose2, (3, 6))
    rig.fill_sentinel()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    want, results = rig.expected(ref.params(camera, **kw))
    rig.compare(rig.outputs(), want, "replay on other images")
    assert [r["status"] for r in results] == [0, ref.PRS_ERR_RANGE]


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_call_level_refusals_write_nothing(hip_ctx):
    depth, pose, camera = sequences(_rng(10), 2, 3, 9, 20, np.float32)
    rig = Rig(hip_ctx, depth, pose, n_images=(3, 3), frame_index=np.tile(np.arange(3, dtype=np.int32), (2, 1)))
    lib, ctx = _lib.load(), hip_ctx._h
    P = lambda **kw: ops.depth_consistency_params(camera, depth_type="f32", **kw)  # noqa: E731
    D = lambda: rig.dcb.descriptor(**rig.inputs())  # noqa: E731

    def run(d, p=None):
        p = P() if p is None else p
        return lib.prs_depth_consistency_batch_run(ctx, C.byref(p) if p != "null" else None, C.byref(d) if d is not None else None)

    rig.fill_sentinel()
    assert run(D()) == 0
    hip_ctx.synchronize()
    rig.fill_sentinel()
    assert run(None) == -1 and run(D(), "null") == -1
    for field in ("depth", "pose", "out", "status", "workspace"):
        d = D()
        setattr(d, field, None)
        assert run(d) == -1, field
    for field, value in (("batch", 0), ("frames", 0), ("rows", 0), ("cols", -1), ("pose_stride", 0), ("pitch", 76), ("pitch", 82),
                         ("out_pitch", 76), ("out_pitch", 81), ("count_pitch", 19)):
        d = D()
        setattr(d, field, value)
        assert run(d) == ref.PRS_ERR_RANGE, (field, value)
    nan, inf = float("nan"), float("inf")
    for field, value in (("window", 0), ("window", 9), ("window", -1), ("stride", 0), ("min_support", -1), ("min_support", 17),
                         ("max_violation", -1), ("max_violation", 17), ("max_rel_diff", -1.0), ("max_rel_diff", nan), ("max_rel_diff", inf),
                         ("depth_scaling_factor_to_meters", 0.0), ("depth_scaling_factor_to_meters", nan), ("fx", inf), ("cy", nan),
                         ("range_min", -1.0), ("range_min", 11.0), ("range_max", inf)):
        p = P()
        setattr(p, field, value)
        assert run(D(), p) == ref.PRS_ERR_RANGE, (field, value)
    p = P()
    p.sensor_in_robot[14] = nan
    assert run(D(), p) == ref.PRS_ERR_RANGE
    for value in (2, -1):
        p = P()
        p.depth_type = value
        assert run(D(), p) == -5, value
    for field, step in (("depth", 2), ("out", 2), ("workspace", 8), ("n_images", 2), ("pose", 2), ("frame_index", 1), ("n_kept", 1),
                        ("n_removed", 2), ("n_skipped", 2), ("status", 2)):
        d = D()
        setattr(d, field, getattr(d, field) + step)
        assert run(d) == -5, field
    # out, support or violation inside depth, before its start but reaching into it, or at its last element
    nbytes = 2 * 3 * 9 * 80
    for field in ("out", "support", "violation"):
        for at in (0, 4, -4, nbytes - 4):
            d = D()
            setattr(d, field, d.depth + at)
            assert run(d) == -5, (field, at)
    # an image side above 2^24, and more elements than 2^31 - 1
    for rows, cols, frames in (((1 << 24) + 1, 1, 1), (1, (1 << 24) + 4, 1), (1 << 10, 1 << 10, 1 << 11)):
        d = D()
        d.rows, d.cols, d.frames, d.pitch, d.out_pitch, d.count_pitch = rows, cols, frames, 4 * cols, 4 * cols, cols
        d.out = d.depth + (1 << 40)  # so that no overlap is what refuses the call
        d.support, d.violation = None, None
        assert run(d) == -5, (rows, cols, frames)
    hip_ctx.synchronize()
    for k, v in rig.outputs().items():
        assert (v.view(np.uint8) == SENTINEL).all(), k


def test_the_python_layer_refuses_what_it_cannot_describe(hip_ctx):
    import torch
    d = ops.DepthConsistencyBatch(2, 2, 5, 6, 2, "f32")
    ok = torch.zeros((2, 2, 5, 6), dtype=torch.float32, device="cuda")
    pose = torch.zeros((2, 2, 16), dtype=torch.float32, device="cuda")
    d.descriptor(ok, pose)
    for bad in (ok.to(torch.float64), ok[..., :5], ok[:, :, :4], ok.transpose(2, 3).contiguous().transpose(2, 3), ok[:, :1].expand(2, 2, 5, 6),
                torch.zeros((2, 2, 5, 6), dtype=torch.uint16, device="cuda")):
        with pytest.raises(ValueError):
            d.descriptor(bad, pose)
    for bad in (pose[:1], pose[..., :12], pose.reshape(2, 2, 4, 4)):
        with pytest.raises(ValueError):
            d.descriptor(ok, bad)
    with pytest.raises(ValueError):
        d.descriptor(ok, pose, n_images=torch.zeros((3,), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        d.descriptor(ok, pose, frame_index=torch.zeros((2, 3), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        d.run(hip_ctx, ops.depth_consistency_params(cases.CAMERA, window=3, depth_type="f32"), ok, pose)
    for bad in (dict(outputs=("supports",)), dict(depth_type="u8"), dict(window=0), dict(window=9), dict(rows=0)):
        with pytest.raises(ValueError):
            ops.DepthConsistencyBatch(**dict(dict(batch=1, frames=1, rows=2, cols=2, window=1), **bad))


# ---- 7. the chain --------------------------------------------------------------------------------------------------------------------
def test_sgm_stereo_speckle_consistency_dense_cloud(hip_ctx):
    """a static stereo camera in front of a wall at a disparity of 4, three pairs of random texture with a tenth of the left pixels
    redrawn: SgmStereoBatch, the speckle filter in place, the consistency filter on that depth, DepthCloudBatch on its out in place.
    The images and the cloud equal the four restatements chained, and the cloud has fewer rows than without the consistency filter"""
    import torch

    import depth_cloud_ref as dref
    import sgm_stereo_ref as sref
    import speckle_ref as fref
    cam = dict(fx=40.0, fy=40.0, cx=30.0, cy=8.0, baseline_m=0.5)  # bf 20: a disparity of 4 is 5 m
    kw = dict(n_disparities=16, min_disparity=0, p1=10, p2=120, n_paths=8, uniqueness_percent=3, lr_max_diff=1)
    B, frames, rows, cols = 1, 3, 21, 70
    rng = _rng(11)
    right = rng.integers(0, 256, (B, frames, rows, cols), dtype=np.uint8)
    left = right[..., np.clip(np.arange(cols) - 4, 0, cols - 1)].copy()
    redraw = rng.random(left.shape) < 0.1
    left[redraw] = rng.integers(0, 256, int(redraw.sum()), dtype=np.uint8)
    pose = np.stack([cases.at(0.002 * i, 0.0, 0.001 * i) for i in range(frames)])[None]
    ckw = dict(range_min=0.1, range_max=10.0, scale=1.0)
    fkw = dict(window=2, stride=1, max_rel_diff=0.05, min_support=2, max_violation=0)  # at a disparity of 4 the sub-pixel part is percents

    stereo = sref.sgm_stereo(left[0], right[0], None, sref.params(20.0, **kw))
    disparity = np.stack([i["disparity"] for i in stereo["results"]])
    depth = np.stack([i["depth"] for i in stereo["results"]])
    speckled = fref.speckle(disparity, depth, None, fref.params(4, 1.0))
    speckled_depth = np.stack([i["companion"] for i in speckled["results"]])
    filtered = ref.depth_consistency(dict(depth=speckled_depth, pose=pose[0]), ref.params(cam, **fkw, **ckw))
    want_depth = np.stack([i["out"] for i in filtered["results"]])
    removed, kept = [i["n_removed"] for i in filtered["results"]], [i["n_kept"] for i in filtered["results"]]
    assert min(removed) > 0 and min(kept) > 0  # the filter has something to remove and something to leave

    dev = torch.device("cuda", 0)
    ds = ops.SgmStereoBatch(B, frames, rows, cols)
    ds.run(hip_ctx, ops.sgm_stereo_params(cam, **kw), torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev))
    sf = ops.SpeckleFilterBatch(B, frames, rows, cols)
    sf.run(hip_ctx, ops.speckle_params(4, 1.0), ds.disparity, ds.depth)
    t_pose = torch.from_numpy(pose).to(dev)
    dcb = ops.DepthConsistencyBatch(B, frames, rows, cols, 2, "f32")
    out = dcb.run(hip_ctx, ops.depth_consistency_params(cam, depth_type="f32", **fkw, **ckw), ds.depth, t_pose)
    n_images = torch.tensor([frames], dtype=torch.int32, device=dev)
    cp = ops.depth_cloud_params(cam, depth_type="f32", **ckw)
    dc = ops.DepthCloudBatch(B, frames, rows, cols, frames * rows * cols)
    dc.run(hip_ctx, cp, out, t_pose, n_images)
    plain = ops.DepthCloudBatch(B, frames, rows, cols, frames * rows * cols)
    plain.count(hip_ctx, cp, ds.depth, t_pose, n_images)
    hip_ctx.synchronize()
    assert out.stride(2) == 72 and out.data_ptr() == dcb._out.data_ptr()
    assert ds.depth.cpu().numpy().tobytes() == speckled_depth[None].tobytes()  # the filter's input is left as it was
    assert dcb.status.cpu().tolist() == [0] and dcb.n_removed.cpu().tolist() == [removed] and dcb.n_kept.cpu().tolist() == [kept]
    assert out.cpu().numpy().tobytes() == want_depth[None].tobytes()
    want = dref.depth_cloud(dict(depth=want_depth, n_images=frames, pose=pose[0]), dref.params(cam, **ckw), dc.out_stride)
    got = dc.cloud_of(0)
    n = want["n_out"]
    assert (got["status"], got["n_out"], got["n_total"]) == (0, n, want["n_total"]) and n == sum(kept)
    assert got["xyz"].tobytes() == want["xyz"][:n].tobytes() and got["row"].tobytes() == want["pixel"][:n].tobytes()
    unfiltered = int(plain.n_total.cpu()[0])
    assert unfiltered == sum(kept) + sum(removed) and 0 < n < unfiltered
