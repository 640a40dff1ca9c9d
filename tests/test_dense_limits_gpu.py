"""The dense image stages (rectifier, depth cloud, dense and semi-global stereo, speckle filter, depth consistency filter) at the two
things that only exist at the batch sizes they are built for.

A. The launch-size guard.  HIP takes no launch of 2^32 or more work-items, 2^24 - 1 workgroups of 256 threads
   (prs_launch_fits, tests/test_launch_fits.py).  Every stage runs, and is right, at the shape that puts its largest launch at that
   count, and refuses the same rig with one image or sequence more with PRS_ERR_UNSUPPORTED before it has written anything.  Both
   rigs are really allocated for their shape, so a missing guard could hand the runtime a launch it does not take, but never
   send a kernel past the end of a buffer.
B. Offsets past 2^32 bytes and 2^31 elements.  Every array of these stages that can pass 2^32 bytes within the stages' cap of
   2^31 - 1 pixels a call does so in one test, and is compared over its whole length.

The inputs are periodic (tests/big_batch.py): P distinct sequences of FRAMES images repeated over the batch on the device, the
last two sequences replaced by two more whose n_images are FRAMES - 1 and 0, so the images a call must not touch lie at the
highest addresses.  The numpy restatements of tests/*_ref.py run on those P + 2 sequences alone, and every output array is
compared with them on the device, byte for byte, pad columns and untouched images (which keep the sentinel) included.  Every test
of B asserts with big_batch.crosses that (a) the last image of the array under test starts at least 4 periods past 2^32 bytes
and (b) an offset that lost 2^32 bytes would land inside another image of the period, so it could not go unnoticed.

Out of scope, because they do not reach 2^32 bytes within the cap or only beyond some 24 GB of device memory: win_r (2 bytes a
pixel), the depth cloud's frame and pixel (4 bytes a point: they share xyz's index), n_valid, status and the other per-image and
per-sequence arrays."""
import ctypes as C
import time

import numpy as np
import pytest

import big_batch as bb
import dense_stereo_ref
import depth_cloud_ref
import depth_consistency_ref
import rectify_ref
import sgm_stereo_ref
import speckle_ref
import test_depth_cloud_gpu as cloud_rig
import test_depth_consistency_gpu as consistency_rig
import test_dense_stereo_gpu as stereo_rig
import test_rectify_gpu as rectify_rig
import test_speckle_gpu as speckle_rig
from srrg2_proslam_amd import _lib, ops

pytestmark = pytest.mark.gpu
F = np.float32
UNSUPPORTED = -5
FRAMES = 3
LIMIT = (1 << 24) - 1  # workgroups of 256 threads in one launch
CAM = stereo_rig.CAM
GB = 1 << 30


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


@pytest.fixture(autouse=True)
def report():
    """prints what the test took: seconds and the peak of device memory"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print("\n[dense limits] %.1f s, peak %.2f GB of device memory" % (time.time() - t0, torch.cuda.max_memory_allocated() / 1e9))
    bb.release()


def counts(P, frames=FRAMES):
    """n_images of the P sequences of the period and of the two behind them"""
    return [frames] * P + [frames - 1, 0]


class Stage:
    """one stage over a periodic batch of B sequences.  A subclass sets: self.t, the device tensors by name, first dimension B;
    self.want, what the call must leave in each, host arrays [P + 2, ...]; self.inplace, by name what the arrays the call works on in place
    held before it, which is what they hold after a refused call (every other array holds the sentinel); and call() -> the status"""

    P = 5

    def compare(self, what=""):
        import torch
        torch.cuda.synchronize()
        for name, t in self.t.items():
            bb.compare_periodic(t, self.want[name][:self.P], "%s %s" % (what, name), self.want[name][self.P:])

    def compare_untouched(self, what=""):
        import torch
        torch.cuda.synchronize()
        for name, t in self.t.items():
            if name in self.inplace:
                bb.compare_periodic(t, self.inplace[name][:self.P], "%s %s" % (what, name), self.inplace[name][self.P:])
            else:
                bb.compare_sentinel("%s %s" % (what, name), t)

    def fill(self):
        bb.fill_sentinel(*[t for name, t in self.t.items() if name not in self.inplace])

    def n_images(self, B, frames):
        self.n_host = counts(self.P, frames)
        n = np.array(self.n_host, np.int32)
        return bb.periodic(n[:self.P], B, n[self.P:])


def put(want, name, seq, f, value, cols):
    if name in want:
        want[name][seq, f, :, :cols] = value


# ---- the stages ----------------------------------------------------------------------------------------------------------------------
class Speckle(Stage):
    """image float32 with `pad` elements behind every row; companion: None or uint16 with a pitch of 2 * cols elements"""

    def __init__(self, ctx, B, rows, cols, pad=0, companion=False, max_size=4, max_diff=1.0, frames=FRAMES, density=0.62):
        self.ctx, S = ctx, self.P + 2
        images = speckle_rig.noise(_rng(31, rows, cols), (S, frames, rows, cols), density)
        full = speckle_rig.padded(images, pad)
        comp = full_comp = None
        if companion:
            comp = _rng(32, rows, cols).integers(1, 9, images.shape).astype(np.uint16)
            full_comp = speckle_rig.padded(comp, cols)
        self.sf = ops.SpeckleFilterBatch(B, frames, rows, cols, ops.SpeckleFilterBatch.OUTPUTS)
        self.t_n = self.n_images(B, frames)
        self.t = dict(image=bb.periodic(full[:self.P], B, full[self.P:]), label=self.sf._label, n_kept=self.sf.n_kept,
                      n_removed=self.sf.n_removed, status=self.sf.status)
        self.inplace = dict(image=full)
        if companion:
            self.t["companion"] = bb.periodic(full_comp[:self.P], B, full_comp[self.P:])
            self.inplace["companion"] = full_comp
        self.p = ops.speckle_params(max_size, max_diff, "f32", "u16" if companion else None)
        self.cols = cols
        want = dict(image=full.copy(), label=bb.sentinel(self.sf._label.shape[1:], np.int32)[None].repeat(S, 0),
                    n_kept=bb.sentinel((S, frames), np.int32), n_removed=bb.sentinel((S, frames), np.int32), status=bb.sentinel((S,), np.int32))
        if companion:
            want["companion"] = full_comp.copy()
        self.removed = 0
        for s in range(S):
            r = speckle_ref.speckle(images[s], comp[s] if companion else None, self.n_host[s], speckle_ref.params(max_size, max_diff))
            want["status"][s] = r["status"]
            for f, image in enumerate(r["results"]):
                if image is not None:
                    for k in ("image", "companion", "label"):
                        put(want, k, s, f, image[k], cols)
                    want["n_kept"][s, f], want["n_removed"][s, f] = image["n_kept"], image["n_removed"]
                    self.removed += image["n_removed"]
        self.want = want

    def call(self):
        d = self.sf.descriptor(self.p, self.t["image"][..., :self.cols], self.t["companion"][..., :self.cols] if "companion" in self.t else None,
                               self.t_n)
        return _lib.load().prs_speckle_batch_run(self.ctx._h, C.byref(self.p), C.byref(d))


class Stereo(Stage):
    """dense (kind "dense") or semi-global ("sgm") stereo.  pitches: those of left and right in bytes, the bytes behind cols random;
    double: "disparity" or "depth", the one output of the run, in a tensor of this rig's with a pitch of 2 * cols floats; outputs:
    those of the batch class, when there is no such one"""

    def __init__(self, ctx, kind, B, rows, cols, pitches=None, double=None, outputs=ops.DenseStereoBatch.OUTPUTS, frames=FRAMES,
                 images_in_flight=None, noise=False, **kw):
        import torch
        self.ctx, self.kind, S = ctx, kind, self.P + 2
        pitches = pitches or (cols, cols)
        left, right = stereo_rig.pairs(_rng(41, rows, cols), (S, frames, rows, cols), noise=noise)
        self.n_disparities = kw["n_disparities"]
        outputs = outputs if double is None else (double, "n_valid")
        if kind == "dense":
            self.ds = ops.DenseStereoBatch(B, frames, rows, cols, outputs)
            self.p, rp = ops.dense_stereo_params(CAM, **kw), dense_stereo_ref.params(F(20.0), **kw)
            run = dense_stereo_ref.dense_stereo
        else:
            self.ds = ops.SgmStereoBatch(B, frames, rows, cols, outputs, images_in_flight=images_in_flight, n_disparities=self.n_disparities)
            self.p, rp = ops.sgm_stereo_params(CAM, **kw), sgm_stereo_ref.params(F(20.0), **kw)
            run = sgm_stereo_ref.sgm_stereo
        assert self.p.bf == 20.0
        self.t_n = self.n_images(B, frames)
        self.images = []
        for i, host in enumerate((left, right)):
            full = _rng(42, i).integers(0, 256, host.shape[:3] + (pitches[i],), dtype=np.uint8)
            full[..., :cols] = host
            self.images.append(bb.periodic(full[:self.P], B, full[self.P:]))
        self.t = dict(n_valid=self.ds.n_valid, status=self.ds.status)
        for name in ("disparity", "depth"):
            if name == double:
                self.t[name] = torch.empty((B, frames, rows, 2 * cols), dtype=torch.float32, device="cuda")
            elif name in outputs:
                self.t[name] = getattr(self.ds, "_" + name)
        self.double, self.cols, self.inplace = double, cols, {}
        want = {name: bb.sentinel((S,) + tuple(t.shape[1:]), F if name in ("disparity", "depth") else np.int32) for name, t in self.t.items()}
        self.valid = 0
        for s in range(S):
            r = run(left[s], right[s], self.n_host[s], rp)
            want["status"][s] = r["status"]
            for f, image in enumerate(r["results"]):
                if image is not None:
                    for k in ("disparity", "depth"):
                        put(want, k, s, f, image[k], cols)
                    want["n_valid"][s, f] = image["n_valid"]
                    self.valid += image["n_valid"]
        self.want = want

    def descriptor(self):
        d = self.ds.descriptor(self.images[0][..., :self.cols], self.images[1][..., :self.cols], self.t_n)
        if self.double:
            setattr(d, self.double, self.t[self.double].data_ptr())
            d.out_pitch = 8 * self.cols
        return d

    def call(self):
        d, lib = self.descriptor(), _lib.load()
        run = lib.prs_dense_stereo_batch_run if self.kind == "dense" else lib.prs_sgm_stereo_batch_run
        return run(self.ctx._h, C.byref(self.p), C.byref(d))


class Consistency(Stage):
    """float32 depth with `pad` valid elements behind every row; wide_counts: support and violation in tensors of this rig's with a
    count_pitch of 4 * cols"""

    def __init__(self, ctx, B, rows, cols, pad=0, wide_counts=False, frames=FRAMES, **kw):
        import torch
        self.ctx, S = ctx, self.P + 2
        depth, pose, camera = consistency_rig.sequences(_rng(51, rows, cols), S, frames, rows, cols, np.float32)
        full = np.concatenate([depth, np.full(depth.shape[:3] + (pad,), 4, F)], -1) if pad else depth
        self.dcb = ops.DepthConsistencyBatch(B, frames, rows, cols, kw["window"], "f32",
                                             ("n_kept", "n_removed", "n_skipped") if wide_counts else ops.DepthConsistencyBatch.OUTPUTS)
        self.p, rp = ops.depth_consistency_params(camera, depth_type="f32", **kw), depth_consistency_ref.params(camera, **kw)
        self.t_n = self.n_images(B, frames)
        self.t_depth, self.t_pose = bb.periodic(full[:self.P], B, full[self.P:]), bb.periodic(pose[:self.P], B, pose[self.P:])
        d = self.dcb
        self.t = dict(out=d._out, n_kept=d.n_kept, n_removed=d.n_removed, n_skipped=d.n_skipped, status=d.status)
        for name in ("support", "violation"):
            self.t[name] = torch.empty((B, frames, rows, 4 * cols), dtype=torch.uint8, device="cuda") if wide_counts else getattr(d, "_" + name)
        self.wide, self.cols, self.inplace = wide_counts, cols, {}
        want = {name: bb.sentinel((S,) + tuple(t.shape[1:]), F if name == "out" else np.uint8 if name in ("support", "violation") else np.int32)
                for name, t in self.t.items()}
        self.support = self.kept = self.removed = 0
        for s in range(S):
            r = depth_consistency_ref.depth_consistency(dict(depth=depth[s], pose=pose[s], n_images=self.n_host[s]), rp)
            want["status"][s], want["n_skipped"][s] = r["status"], r["n_skipped"]
            for f, image in enumerate(r["results"]):
                if image is not None:
                    for k in ("out", "support", "violation"):
                        put(want, k, s, f, image[k], cols)
                    want["n_kept"][s, f], want["n_removed"][s, f] = image["n_kept"], image["n_removed"]
                    self.support += int(image["support"].sum())
                    self.kept, self.removed = self.kept + image["n_kept"], self.removed + image["n_removed"]
        self.want = want

    def call(self):
        d = self.dcb.descriptor(self.t_depth[..., :self.cols], self.t_pose, self.t_n)
        if self.wide:
            d.support, d.violation, d.count_pitch = self.t["support"].data_ptr(), self.t["violation"].data_ptr(), 4 * self.cols
        return _lib.load().prs_depth_consistency_batch_run(self.ctx._h, C.byref(self.p), C.byref(d))


class Cloud(Stage):
    """float32 depth with `pad` valid elements behind every row, every `step`-th pixel; a sequence has room for all its samples"""

    def __init__(self, ctx, B, rows, cols, pad=0, step=1, frames=FRAMES):
        self.ctx, S = ctx, self.P + 2
        self.n_host = counts(self.P, frames)
        rng = _rng(61, rows, cols)
        seqs = [cloud_rig.sequence(rng, frames, rows, cols, "f32", n_images=n) for n in self.n_host]
        self.out_stride = frames * ((rows + step - 1) // step) * ((cols + step - 1) // step)
        self.dc = ops.DepthCloudBatch(B, frames, rows, cols, self.out_stride)
        self.p, rp = ops.depth_cloud_params(cloud_rig.K, depth_type="f32", step=step), depth_cloud_ref.params(cloud_rig.K, step=step)
        full = np.full((S, frames, rows, cols + pad), 1.5, F)
        full[..., :cols] = np.stack([s["depth"] for s in seqs])
        pose = np.stack([s["pose"] for s in seqs])
        self.t_depth, self.t_pose = bb.periodic(full[:self.P], B, full[self.P:]), bb.periodic(pose[:self.P], B, pose[self.P:])
        self.t_n = self.n_images(B, frames)
        d = self.dc
        self.t = dict(xyz=d.xyz, frame=d.node, pixel=d.row, n_out=d.n_out, n_total=d.n_total, n_skipped=d.n_skipped, status=d.status)
        self.cols, self.inplace = cols, {}
        n = self.out_stride
        before = dict(xyz=bb.sentinel((n, 4), F), frame=bb.sentinel((n,), np.int32), pixel=bb.sentinel((n,), np.int32))
        results = [depth_cloud_ref.depth_cloud(s, rp, n, before) for s in seqs]
        self.want = {name: np.stack([np.asarray(r[name], F if name == "xyz" else np.int32) for r in results]) for name in self.t}
        self.kept = sum(r["n_out"] for r in results)

    def call(self):
        d = self.dc.descriptor(self.t_depth[..., :self.cols], self.t_pose, self.t_n)
        return _lib.load().prs_depth_cloud_batch_run(self.ctx._h, C.byref(self.p), C.byref(d))


class Rectify(Stage):
    """B images (the items are images here, and no call leaves any out) through two maps that alternate unevenly over the period;
    src_pitch, dst_pitch in elements"""

    def __init__(self, ctx, B, shape, np_dtype=np.uint8, interpolation="bilinear", src_pitch=None, dst_pitch=None, kinds=("euroc", "wide")):
        import torch
        self.ctx, P = ctx, self.P
        rows, cols = shape
        sp, dp = src_pitch or cols, dst_pitch or cols
        src = rectify_rig.image(_rng(71, rows, cols), shape, np_dtype, batch=P)
        maps = [rectify_rig.make_map(kind, shape) for kind in kinds]
        map_of = np.array([0, 1, 1, 0, 1][:P], np.int32)
        type_name = {np.uint8: "u8", np.uint16: "u16", np.float32: "f32"}[np_dtype]
        self.p = ops.rectify_params(type_name, interpolation, border=9)
        full = _rng(72).integers(1, 200, (P, rows, sp)).astype(np_dtype)
        full[..., :cols] = src
        self.t_src, self.t_map_of = bb.periodic(full, B), bb.periodic(map_of, B)
        arr = (_lib.RectifyMap * len(maps))(*[m.struct() for m in maps])
        self.t_maps = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).cuda()
        tdtype = {np.uint8: torch.uint8, np.uint16: torch.uint16, np.float32: torch.float32}[np_dtype]
        self.t = dict(dst=torch.empty((B, rows, dp), dtype=tdtype, device="cuda"), n_border=torch.empty((B,), dtype=torch.int32, device="cuda"),
                      status=torch.empty((B,), dtype=torch.int32, device="cuda"))
        self.inplace = {}
        dst, n_border, status = rectify_ref.rectify_batch(src, maps, map_of, None, interpolation, 9)
        want_dst = bb.sentinel((P, rows, dp), np_dtype)
        want_dst[..., :cols] = dst
        self.want = dict(dst=want_dst, n_border=np.asarray(n_border, np.int32), status=np.asarray(status, np.int32))
        self.border = int(np.sum(n_border))
        self.B, self.shape, self.sp, self.dp, self.es, self.n_maps = B, shape, sp, dp, np.dtype(np_dtype).itemsize, len(maps)

    def call(self):
        d = _lib.RectifyBatch()
        rows, cols = self.shape
        d.batch, d.src_rows, d.src_cols, d.src_pitch, d.src = self.B, rows, cols, self.sp * self.es, self.t_src.data_ptr()
        d.dst_rows, d.dst_cols, d.dst_pitch, d.dst = rows, cols, self.dp * self.es, self.t["dst"].data_ptr()
        d.n_maps, d.maps, d.map_of = self.n_maps, self.t_maps.data_ptr(), self.t_map_of.data_ptr()
        d.n_border, d.status = self.t["n_border"].data_ptr(), self.t["status"].data_ptr()
        return _lib.load().prs_rectify_batch_run(self.ctx._h, C.byref(self.p), C.byref(d))


# ---- A. the launch-size guard ----------------------------------------------------------------------------------------------------------
# 1 x 1 images: a stage's largest launch has one workgroup an image (two for the census), or one a sequence's chunk
SEQUENCES = LIMIT // FRAMES
assert SEQUENCES * FRAMES == LIMIT
STEREO = dict(n_disparities=16, min_disparity=0, uniqueness_percent=10, lr_max_diff=1)
LIMIT_RIGS = {
    # speckle: tile, flatten and apply launch a workgroup an image
    "speckle": lambda ctx, more: Speckle(ctx, SEQUENCES + more, 1, 1, max_size=1),
    # the census launches two workgroups an image: 2^24 - 2 with 2^23 - 1 images, one image a sequence
    "dense_stereo": lambda ctx, more: Stereo(ctx, "dense", (LIMIT // 2) + more, 1, 1, frames=1, aggregation_radius=1, **STEREO),
    "sgm_stereo": lambda ctx, more: Stereo(ctx, "sgm", (LIMIT // 2) + more, 1, 1, frames=1, p1=10, p2=120, n_paths=8, **STEREO),
    # the filter launches a workgroup an image, prepare one a sequence
    "depth_consistency": lambda ctx, more: Consistency(ctx, SEQUENCES + more, 1, 1, window=1, min_support=1),
    # both passes launch a workgroup a chunk of 1024 samples, here one an image; the scan one a sequence
    "depth_cloud": lambda ctx, more: Cloud(ctx, SEQUENCES + more, 1, 1),
    # one tile an image and, with PRS_RECTIFY_CHUNK=1, one image a workgroup
    "rectify": lambda ctx, more: Rectify(ctx, LIMIT + more, (1, 1), dst_pitch=4),
}


@pytest.fixture
def one_image_a_workgroup(monkeypatch):
    monkeypatch.setenv("PRS_RECTIFY_CHUNK", "1")


@pytest.mark.parametrize("stage", sorted(LIMIT_RIGS))
def test_the_largest_launch_that_fits_runs_and_is_right(hip_ctx, one_image_a_workgroup, stage):
    assert _lib.load().prs_launch_fits(LIMIT, 256) == 1
    bb.need_memory(6 * GB)
    rig = LIMIT_RIGS[stage](hip_ctx, 0)
    rig.fill()
    assert rig.call() == 0
    rig.compare(stage)
    del rig


@pytest.mark.parametrize("stage", sorted(LIMIT_RIGS))
def test_one_more_is_refused_and_nothing_is_written(hip_ctx, one_image_a_workgroup, stage):
    """the same rig with one sequence more (the rectifier: one image), allocated for that: PRS_ERR_UNSUPPORTED, and every output
    holds the sentinel, also those an earlier launch of the stage would have written"""
    assert _lib.load().prs_launch_fits(LIMIT + 1, 256) == 0
    bb.need_memory(6 * GB)
    rig = LIMIT_RIGS[stage](hip_ctx, 1)
    rig.fill()
    assert rig.call() == UNSUPPORTED
    rig.compare_untouched(stage)
    del rig


# ---- B. offsets past 2^32 bytes ----------------------------------------------------------------------------------------------------------
ROWS, COLS = 21, 70  # an image: 1470 pixels, neither a power of two nor a multiple of a tile
PIXELS = ROWS * COLS


def sequences_for(pixels, per_image=PIXELS, frames=FRAMES, margin=1.03):
    """the least batch whose images hold `pixels` pixels and a margin"""
    return int(pixels * margin) // (per_image * frames) + 1


def crossing(rig, rows, what, frames=FRAMES):
    """big_batch.crosses for each (name, bytes an image, element bytes or None) of rows: the arrays under test of one run"""
    images = int(next(iter(rig.t.values())).shape[0]) * frames
    for name, image_bytes, element in rows:
        bb.crosses("%s %s" % (what, name), images, image_bytes, frames * rig.P, element, element is not None)


def test_speckle_past_4_gib(hip_ctx):
    """parent, size and label (4 bytes a pixel), the float32 image with a pad element a row, and a uint16 companion with a pitch of
    2 * cols elements: all of them pass 2^32 bytes at 2^30 pixels"""
    B = sequences_for(1 << 30)
    bb.need_memory(23 * GB)
    rig = Speckle(hip_ctx, B, ROWS, COLS, pad=1, companion=True)
    crossing(rig, (("parent", PIXELS * 4, None), ("size", PIXELS * 4, None), ("label", ROWS * 72 * 4, None),
                   ("image", ROWS * (COLS + 1) * 4, None), ("companion", ROWS * 2 * COLS * 2, None)), "speckle")
    assert rig.t["image"].stride(2) == COLS + 1 and rig.t["companion"].stride(2) == 2 * COLS and rig.removed > 100
    rig.fill()
    assert rig.call() == 0
    rig.compare("speckle")
    del rig


@pytest.mark.parametrize("kind", ["dense", "sgm"])
@pytest.mark.parametrize("layout", ["census", "disparity", "depth", "left", "right"])
def test_stereo_past_4_gib(hip_ctx, kind, layout):
    """census: the census words of both images and the records (8 bytes a pixel) pass 2^32 bytes at 2^29 pixels; disparity,
    depth: the one output of the run with a pitch of 2 * cols floats; left, right: that image with a pitch of 8 * cols bytes (one a
    run, and the disparity alone, keep a run at some 24 GB).  lr_max_diff 1: the right-reference match and win_r are read at the high indices too.  Few disparities (and 4 paths) keep the
    semi-global volume and the time small"""
    B = sequences_for(1 << 29)
    bb.need_memory(25 * GB)
    kw = dict(STEREO, aggregation_radius=3) if kind == "dense" else dict(STEREO, p1=10, p2=120, n_paths=4)
    pitches = (8 * COLS if layout == "left" else COLS + 3, 8 * COLS if layout == "right" else COLS + 1)
    rig = Stereo(hip_ctx, kind, B, ROWS, COLS, pitches, double=layout if layout in ("disparity", "depth") else None,
                 outputs=ops.DenseStereoBatch.OUTPUTS if layout == "census" else ("disparity", "n_valid"), **kw)
    rows = dict(census=(("census_l", PIXELS * 8, None), ("census_r", PIXELS * 8, None), ("records", PIXELS * 8, None)),
                disparity=(("disparity", ROWS * 2 * COLS * 4, None),), depth=(("depth", ROWS * 2 * COLS * 4, None),),
                left=(("left", ROWS * 8 * COLS, None),), right=(("right", ROWS * 8 * COLS, None),))[layout]
    crossing(rig, rows, "%s stereo" % kind)
    assert rig.valid > 1000
    rig.fill()
    assert rig.call() == 0
    rig.compare("%s stereo, %s" % (kind, layout))
    del rig


@pytest.mark.parametrize("n_disparities", [256, 254])
def test_sgm_volume_past_4_gib(hip_ctx, n_disparities):
    """the S volume (2 bytes an entry) of every image of the call at once, images_in_flight given above the 2 GiB budget: 2^31
    entries and 2^32 bytes.  256: a lane's four disparities are one 8-byte word; 254: they move singly and the right-winner stage
    loads two.  8 paths, lr_max_diff 1"""
    rows, cols = 48, 131
    volume = rows * cols * n_disparities * 2
    B = sequences_for(1 << 31, rows * cols * n_disparities, margin=1.06)
    bb.need_memory(8 * GB)
    rig = Stereo(hip_ctx, "sgm", B, rows, cols, images_in_flight=B * FRAMES, n_disparities=n_disparities, min_disparity=0, p1=10, p2=120,
                 n_paths=8, uniqueness_percent=10, lr_max_diff=1)
    assert rig.ds.images_in_flight == B * FRAMES and rig.descriptor().images_in_flight == B * FRAMES  # one chunk
    assert B * FRAMES > ops.sgm_stereo_images_in_flight(B, FRAMES, rows, cols, n_disparities)            # above the budget's
    crossing(rig, (("volume", volume, 2),), "sgm volume")
    assert rig.valid > 1000
    rig.fill()
    assert rig.call() == 0
    rig.compare("sgm volume, %d disparities" % n_disparities)
    del rig


def test_depth_consistency_past_4_gib(hip_ctx):
    """depth (three pad elements a row) and out, float32, pass 2^32 bytes at 2^30 pixels, and so does the neighbour's row
    grow * pitch; support and violation with a count_pitch of 4 * cols.  The poses are those of the stage's own tests: neighbours
    are read and vote"""
    B = sequences_for(1 << 30)
    bb.need_memory(23 * GB)
    rig = Consistency(hip_ctx, B, ROWS, COLS, pad=3, wide_counts=True, window=2, min_support=1)
    crossing(rig, (("depth", ROWS * (COLS + 3) * 4, None), ("out", ROWS * 72 * 4, None), ("support", ROWS * 4 * COLS, None),
                   ("violation", ROWS * 4 * COLS, None)), "depth consistency")
    assert rig.support > 1000 and rig.kept > 1000 and rig.removed > 1000
    rig.fill()
    assert rig.call() == 0
    rig.compare("depth consistency")
    del rig


def test_depth_cloud_past_4_gib(hip_ctx):
    """step 2 on float32 depth of 2^30 pixels (a pad element a row): the depth passes 2^32 bytes, and xyz, 16 bytes a row with room
    for a quarter of the pixels, does so as well"""
    B = sequences_for(1 << 30)
    bb.need_memory(16 * GB)
    rig = Cloud(hip_ctx, B, ROWS, COLS, pad=1, step=2)
    assert rig.out_stride == FRAMES * 11 * 35 and B * rig.out_stride > 1 << 28 and rig.kept > 1000
    crossing(rig, (("depth", ROWS * (COLS + 1) * 4, None),), "depth cloud")
    bb.crosses("depth cloud xyz", B, rig.out_stride * 16, rig.P)  # a sequence's rows
    rig.fill()
    assert rig.call() == 0
    rig.compare("depth cloud")
    del rig


RECTIFY = {
    # (element, interpolation, src pitch and dst pitch in elements): staged footprints need a source pitch of a multiple of 16 bytes
    "u8_staged": (np.uint8, "bilinear", 144, 132),
    "u8_from_global": (np.uint8, "bilinear", 135, 134),
    "u16_nearest": (np.uint16, "nearest", 134, 132),
    "f32_nearest": (np.float32, "nearest", 133, 132),
}


@pytest.mark.parametrize("case", sorted(RECTIFY))
def test_rectify_past_4_gib(hip_ctx, case):
    """src and dst pass 2^32 bytes each; two maps through map_of, so the period covers the switch of a workgroup's map"""
    np_dtype, interpolation, sp, dp = RECTIFY[case]
    rows, cols, es = 48, 131, np.dtype(np_dtype).itemsize
    B = int((1 << 32) * 1.03) // (rows * min(sp, dp) * es) + 1
    bb.need_memory(12 * GB)
    rig = Rectify(hip_ctx, B, (rows, cols), np_dtype, interpolation, sp, dp)
    assert (rig.t_src.data_ptr() % 16 == 0 and sp * es % 16 == 0) == (case == "u8_staged") or es > 1
    for name, pitch in (("src", sp), ("dst", dp)):
        bb.crosses("rectify %s %s" % (case, name), B, rows * pitch * es, rig.P)
    assert 0 < rig.border < rig.P * rows * cols
    rig.fill()
    assert rig.call() == 0
    rig.compare("rectify %s" % case)
    del rig
