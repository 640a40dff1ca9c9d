"""Depth normals on the device (ops.DepthNormalsBatch: prs_depth_normals_batch_run) against the numpy restatement
(tests/depth_normals_ref.py).  Every output array is compared byte for byte over its whole length: both sides do the same IEEE
operations in the same order, so no tolerance is involved, and what a call must not touch -- the images from n_images on, refused
sequences, the cloud rows outside [row_base, row_n) -- is compared with the sentinel it was filled with.  TW x TH is the kernel's
tile."""
import ctypes as C

import numpy as np
import pytest

import depth_cloud_ref as cloud_ref
import depth_normals_cases as cases
import depth_normals_ref as ref
from srrg2_proslam_amd import _lib_normals, ops

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0xA5
TW, TH = 64, 16
K = cases.K
SETTINGS = ((1, 0), (2, 1), (8, 0), (8, 3), (1, 3))


def _rng(*seed):
    return np.random.default_rng(list(seed))


def sentinel(shape, dtype):
    return np.full(tuple(shape) + (np.dtype(dtype).itemsize,), SENTINEL, np.uint8).view(dtype).reshape(shape)


def poses(rng, n, far=0.0):
    """n rigid float32 poses [n, 16]: any rotation, a translation of a few metres plus `far`"""
    out = np.zeros((n, 4, 4), F)
    for i in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        out[i, :3, :3] = q * np.sign(np.linalg.det(q))
        out[i, :3, 3] = rng.uniform(-5, 5, 3) + far
        out[i, 3, 3] = 1
    return out.reshape(n, 16)


def sequence(rng, frames, rows, cols, depth_type, n_images=None, pose_stride=None, index=False):
    s = dict(depth=cases.random_depth(rng, (frames, rows, cols), depth_type), n_images=n_images,
             pose=poses(rng, frames if pose_stride is None else pose_stride))
    if index:
        s["frame_index"] = rng.permutation(s["pose"].shape[0])[:frames].astype(np.int32)
    return s


class Rig:
    """an ops.DepthNormalsBatch over device copies of a list of sequences in the restatement's layout (all of one shape; n_images and
    frame_index set in all or in none).  pad: elements behind every image row, filled with depths that would be valid neighbours.
    row_stride: the batch also owns rows, and the rig a real ops.DepthCloudBatch of that out_stride over the same images"""

    def __init__(self, ctx, seqs, depth_type, pad=0, row_stride=None, outputs=ops.DepthNormalsBatch.OPTIONAL):
        import torch
        self.ctx, self.seqs, self.B, self.depth_type, self.pad = ctx, seqs, len(seqs), depth_type, pad
        self.frames, self.rows, self.cols = seqs[0]["depth"].shape
        self.scale = 1e-3 if depth_type == "u16" else 1.0
        self.dev = torch.device("cuda", 0)
        self.nb = ops.DepthNormalsBatch(self.B, self.frames, self.rows, self.cols, row_stride, outputs)
        self.cloud = ops.DepthCloudBatch(self.B, self.frames, self.rows, self.cols, row_stride) if row_stride else None
        self.t = {}
        self.upload()

    def _put(self, name, host):
        import torch
        host = np.ascontiguousarray(host)
        if name in self.t and tuple(self.t[name].shape) == host.shape:
            self.t[name].copy_(torch.from_numpy(host))
        else:
            self.t[name] = torch.from_numpy(host).to(self.dev)

    def upload(self, seqs=None):
        self.seqs = self.seqs if seqs is None else seqs
        s0 = self.seqs[0]
        u16 = self.depth_type == "u16"
        depth = np.full((self.B, self.frames, self.rows, self.cols + self.pad), 2000 if u16 else 2.0, np.uint16 if u16 else F)
        depth[..., :self.cols] = np.stack([s["depth"] for s in self.seqs])
        self._put("depth", depth)
        self._put("pose", np.stack([np.asarray(s["pose"], F).reshape(-1, 16) for s in self.seqs]))
        self._put("n_full", np.array([self.frames if s.get("n_images") is None else s["n_images"] for s in self.seqs], np.int32))
        if s0.get("n_images") is not None:
            self._put("n_images", np.array([s["n_images"] for s in self.seqs], np.int32))
        if s0.get("frame_index") is not None:
            self._put("frame_index", np.stack([np.asarray(s["frame_index"], np.int32) for s in self.seqs]))

    def inputs(self):
        t = self.t
        return dict(depth=t["depth"][..., :self.cols], pose=t["pose"], n_images=t.get("n_images"), frame_index=t.get("frame_index"))

    def tensors(self):
        names = ("normal", "n_normal", "status", "row_normal", "n_bad_rows")
        return {k: getattr(self.nb, k) for k in names if getattr(self.nb, k) is not None}

    def fill_sentinel(self):
        import torch
        for t in self.tensors().values():
            t.view(torch.uint8).fill_(SENTINEL)

    def outputs(self):
        return {k: t.cpu().numpy() for k, t in self.tensors().items()}

    def params(self, radius, smooth, **kw):
        kw.setdefault("scale", self.scale)
        camera = kw.pop("camera", K)
        return ops.depth_normals_params(camera, radius, smooth, depth_type=self.depth_type, **kw), ref.params(camera, radius, smooth, **kw)

    def run_cloud(self, append=False, **kw):
        """the real cloud of the images as they stand -> its rows on the host, per sequence, for the restatement"""
        kw.setdefault("scale", self.scale)
        cp = ops.depth_cloud_params(K, depth_type=self.depth_type, **kw)
        i = self.inputs()
        self.cloud.run(self.ctx, cp, i["depth"], i["pose"], self.t["n_full"], i["frame_index"], append=append)
        self.ctx.synchronize()
        return self.host_rows()

    def host_rows(self, bases=None):
        c = self.cloud
        frame, pixel, n = c.node.cpu().numpy(), c.row.cpu().numpy(), c.n_out.cpu().numpy()
        return [dict(frame=frame[b], pixel=pixel[b], n=int(n[b]), base=None if bases is None else int(bases[b])) for b in range(self.B)]

    def expected(self, rp, rows=None, before=None):
        out = []
        for b, s in enumerate(self.seqs):
            was = dict(normal=sentinel((self.frames, self.rows, self.cols, 4), F), n_normal=sentinel((self.frames,), np.int32))
            if rows is not None:
                was["row_normal"] = sentinel((self.nb.row_stride, 4), F)
            if before is not None:
                was.update({k: v[b] for k, v in before.items()})
            out.append(ref.depth_normals(s, rp, was, None if rows is None else rows[b]))
        return out

    def compare(self, got, want, what=""):
        for b, w in enumerate(want):
            assert int(got["status"][b]) == w["status"], (what, b, "status", int(got["status"][b]), w["status"])
            for k in ("normal", "n_normal", "row_normal"):
                if k in got and k in w:
                    if got[k][b].tobytes() != w[k].tobytes():
                        g, x = got[k][b].reshape(-1), w[k].reshape(-1)
                        at = int(np.flatnonzero(g.view(np.uint32) != x.view(np.uint32))[0])
                        raise AssertionError("%s: sequence %d, %s differs first at element %d of %s: got %r, want %r"
                                             % (what, b, k, at, got[k][b].shape, g[at], x[at]))
            if "n_bad_rows" in got and "n_bad_rows" in w:
                bad = sentinel((1,), np.int32)[0] if w["n_bad_rows"] is None else w["n_bad_rows"]
                assert int(got["n_bad_rows"][b]) == bad, (what, b, "n_bad_rows", int(got["n_bad_rows"][b]), bad)

    def check(self, radius, smooth, what="", rows=None, append=False, before=None, **kw):
        """run and compare every sequence with the restatement; rows: host_rows() of the cloud the rig has run -> the restatement's"""
        p, rp = self.params(radius, smooth, **kw)
        if before is None:
            self.fill_sentinel()
        i = self.inputs()
        if rows is None:
            self.nb.run(self.ctx, p, i["depth"], n_images=i["n_images"])
        else:
            self.nb.run(self.ctx, p, cloud=self.cloud, append=append, **i)
        self.ctx.synchronize()
        want = self.expected(rp, rows, before)
        self.compare(self.outputs(), want, "%s radius %d smooth %d" % (what, radius, smooth))
        return want


# ---- 1. shapes, types, pitches, settings --------------------------------------------------------------------------------------------
# 1 x 1, 1 x 2, 2 x 1; 3 x 3; exactly a tile; a tile and one more row and column; several tiles with ragged edges; narrower than radius 8
SHAPES = [(1, 1), (1, 2), (2, 1), (3, 3), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 2), (40, 5)]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("depth_type", ["u16", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_types_pitches_and_settings(hip_ctx, shape, depth_type, pad):
    rows, cols = shape
    seqs = [sequence(_rng(1, rows, cols, b), 2, rows, cols, depth_type) for b in range(2)]
    rig = Rig(hip_ctx, seqs, depth_type, pad=pad)
    assert rig.inputs()["depth"].stride(2) == cols + pad
    for r, s in SETTINGS:
        want = rig.check(r, s, "%dx%d %s" % (rows, cols, depth_type))
        assert all(w["status"] == ref.PRS_OK for w in want)
        if rows >= TH and cols >= TW and r < 8:
            found = np.mean([(w["normal"][..., 3] > 0).mean() for w in want])
            assert 0.3 < found < 0.98, found  # the images exercise both outcomes


def test_every_neighbour_count_and_both_orientations_occur(hip_ctx):
    """the image of the shapes test reaches every branch of the rule: w = 2, 3 and 4, normals that were flipped and that were not"""
    s = sequence(_rng(1, 1), 1, 2 * TH + 1, 2 * TW + 2, "f32")
    p = ref.params(K, 2, 0)
    d = ref.metres(s["depth"][0], p)
    n, w, has = ref.raw_normals(d, p)
    assert {2.0, 3.0, 4.0} <= set(np.unique(w[has]).tolist())
    p_open = ref.params(K, 2, 0, max_rel_diff=10.0)
    assert (ref.raw_normals(d, p_open)[1] > w).any()  # the gate closes on some neighbours
    Rig(hip_ctx, [s], "f32").check(2, 0, max_rel_diff=10.0)


# ---- 2. the halo: a depth step exactly on a tile seam ----------------------------------------------------------------------------------
@pytest.mark.parametrize("vertical", [True, False], ids=["vertical", "horizontal"])
def test_a_depth_step_on_a_tile_seam(hip_ctx, vertical):
    """2 m | 3 m with the step between the first and the second tile, radius 8 and a 7 x 7 window: the tangents and the window of the
    pixels up to 11 from the seam read the other tile through the halo, and the gate keeps them apart"""
    rows, cols = 2 * TH + 5, 2 * TW + 7
    tilt = cases.plane_depth(rows, cols, K, (0.2, -0.1, 1.0), 2.0)[0]
    step = cases.step_image(rows, cols, 1.0, 1.5, TW if vertical else TH, vertical)
    depth = (tilt * step).astype(F)
    rig = Rig(hip_ctx, [dict(depth=depth[None], n_images=None, pose=poses(_rng(2), 1))], "f32")
    want = rig.check(8, 3, "seam")[0]["normal"][0]
    at = TW if vertical else TH
    near = want[:, at - 11:at + 11] if vertical else want[at - 11:at + 11]
    assert (near[..., 3] > 0).all() and (want[..., 3] == 4).any() and (near[..., 3] == 3).any()
    # the gate held: every normal is the plane's, also beside the step (a difference across it would tilt by tens of degrees)
    truth = cases.plane_depth(rows, cols, K, (0.2, -0.1, 1.0), 2.0)[1]
    assert ref.angle_between(near[..., :3], truth).max() < 1e-3
    rig.check(8, 3, "seam, gate open", max_rel_diff=0.6)  # and with the gate open the halo's values enter the sums
    rig.check(8, 0, "seam, no smoothing")


# ---- 3. n_images, refusals per sequence, odd values, denormals, optional outputs -------------------------------------------------------
@pytest.mark.parametrize("depth_type", ["u16", "f32"])
def test_n_images_below_frames_leaves_the_tail(hip_ctx, depth_type):
    seqs = [sequence(_rng(3, b), 4, 9, 70, depth_type, n_images=n) for b, n in enumerate((0, 1, 3, 4))]
    want = Rig(hip_ctx, seqs, depth_type).check(2, 1, "n_images")
    for w, n in zip(want, (0, 1, 3, 4)):
        assert (w["normal"][n:].view(np.uint8) == SENTINEL).all() and (w["n_normal"][n:].view(np.uint8) == SENTINEL).all()
        assert all(w["n_normal"][f] > 0 for f in range(n))


def test_a_batch_with_a_refused_sequence(hip_ctx):
    seqs = [sequence(_rng(4, b), 3, 20, 66, "u16", n_images=n) for b, n in enumerate((3, -1, 4, 2))]
    want = Rig(hip_ctx, seqs, "u16").check(2, 1, "refused")
    assert [w["status"] for w in want] == [0, ref.PRS_ERR_RANGE, ref.PRS_ERR_RANGE, 0]
    for b in (1, 2):
        assert (want[b]["normal"].view(np.uint8) == SENTINEL).all() and (want[b]["n_normal"].view(np.uint8) == SENTINEL).all()


def test_values_that_are_not_depths(hip_ctx):
    d, odd = cases.odd_values_image(_rng(5))
    rig = Rig(hip_ctx, [dict(depth=d[None], n_images=None, pose=poses(_rng(5), 1))], "f32")
    for r, s in ((1, 0), (1, 1), (2, 3)):
        got = rig.check(r, s, "odd values")[0]["normal"][0]
        assert not got[odd].any() and (got[~odd][:, 3] > 0).any()
    rig.check(1, 1, "odd values, gate above 1", max_rel_diff=2.0, range_min=0.0)  # a hole's 0 would pass |0 - d| <= 2 d
    u = np.full((3, 8), 1000, np.uint16)
    u[1] = [0, 1, 499, 500, 2000, 2001, 65535, 1000]
    rig = Rig(hip_ctx, [dict(depth=u[None], n_images=None, pose=poses(_rng(5), 1))], "u16")
    got = rig.check(1, 0, "u16 edges", range_min=0.5, range_max=2.0, max_rel_diff=10.0)[0]["normal"][0]
    assert got[0, :, 3].tolist() == [0, 0, 0, 3, 3, 0, 0, 2]


def test_a_valid_depth_of_zero(hip_ctx):
    """scale * raw underflows to 0 and range_min is 0: the pixel is valid, a usable neighbour of other such pixels, and its point is
    the origin, so it has no normal -- on both sides"""
    d = np.full((6, 8), 2.0, F)
    d[2:5, 2:6] = 1e-40  # a denormal; times 1e-6 it is below half the least denormal
    rig = Rig(hip_ctx, [dict(depth=d[None], n_images=None, pose=poses(_rng(5), 1))], "f32")
    got = rig.check(1, 1, "zero depth", scale=1e-6, range_min=0.0)[0]["normal"][0]
    assert not got[2:5, 2:6].any() and (got[0, :, 3] > 0).all()


def test_products_that_are_denormal(hip_ctx):
    """the device keeps float32 denormals as numpy does: a len2 that is a denormal gives a normal, one that underflows to 0 none"""
    d = np.full((4, 70), 1.0, F)
    rig = Rig(hip_ctx, [dict(depth=d[None], n_images=None, pose=poses(_rng(5), 1))], "f32")
    for s in (0, 1):
        got = rig.check(1, s, "denormal len2", camera=dict(fx=3e10, fy=3e10, cx=0.0, cy=0.0))[0]["normal"][0]
        assert (got[..., 3] > 0).all() and np.abs(got[..., 2] + 1).max() < 1e-3  # a denormal len2 holds ten bits in the corners
        got = rig.check(1, s, "len2 underflows", camera=dict(fx=1e18, fy=1e18, cx=0.0, cy=0.0))[0]["normal"][0]
        assert not got.any()
    # denormal components that survive to the output: a plane tilted by 1e-39 per metre cannot be told from the axis, but the
    # products on the way are denormal and must not be flushed
    tilt = (1.0 + 1e-7 * np.arange(70, dtype=np.float64))[None, :].repeat(4, 0).astype(F)
    rig.upload([dict(depth=tilt[None], n_images=None, pose=poses(_rng(5), 1))])
    rig.check(1, 0, "tiny tilt", camera=dict(fx=3e10, fy=3e10, cx=0.0, cy=0.0))


@pytest.mark.parametrize("outputs", [(), ("n_normal",)])
@pytest.mark.parametrize("with_rows", [False, True])
def test_each_subset_of_the_optional_outputs(hip_ctx, outputs, with_rows):
    seqs = [sequence(_rng(6, b), 2, 18, 66, "u16") for b in range(2)]
    rig = Rig(hip_ctx, seqs, "u16", row_stride=2 * 18 * 66 if with_rows else None, outputs=outputs)
    assert (rig.nb.n_normal is not None) == ("n_normal" in outputs) and (rig.nb.row_normal is not None) == with_rows
    rows = rig.run_cloud() if with_rows else None
    want = rig.check(2, 1, "outputs %s" % (outputs,), rows=rows)
    if with_rows:
        assert all(w["n_bad_rows"] == 0 for w in want) and min(r["n"] for r in rows) > 1000


# ---- 4. cloud rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth_type", ["u16", "f32"])
@pytest.mark.parametrize("step", [1, 3])
def test_rows_behind_a_real_cloud(hip_ctx, step, depth_type):
    frames, rows, cols = 3, 20, 70
    seqs = [sequence(_rng(7, b), frames, rows, cols, depth_type, pose_stride=5, index=True) for b in range(2)]
    stride = frames * len(range(0, rows, step)) * len(range(0, cols, step)) + 300  # 256 rows a workgroup: the last one is ragged
    rig = Rig(hip_ctx, seqs, depth_type, row_stride=stride)
    cloud_rows = rig.run_cloud(step=step)
    want = rig.check(2, 1, "rows step %d" % step, rows=cloud_rows)
    for w, r in zip(want, cloud_rows):
        n = r["n"]
        assert w["n_bad_rows"] == 0 and 300 < n < stride - 256
        assert (w["row_normal"][n:].view(np.uint8) == SENTINEL).all()
        found = w["row_normal"][:n, 3] > 0
        assert 0.3 < found.mean() < 1.0
        # a rotation keeps the length
        assert np.abs(np.linalg.norm(w["row_normal"][:n][found][:, :3].astype(np.float64), axis=1) - 1).max() < 1e-5
    assert rig.nb.n_rows.cpu().tolist() == [r["n"] for r in cloud_rows]


def test_rows_with_a_sensor_offset_far_from_the_origin_and_a_large_rotation(hip_ctx):
    seqs = [sequence(_rng(8, b), 2, 18, 66, "f32") for b in range(2)]
    for s in seqs:
        s["pose"] = poses(_rng(8, 9), 2, far=1e6)
        s["pose"].reshape(-1, 4, 4)[0, :3, :3] = F([[-1, 0, 0], [0, -0.99985, 0.0173], [0, 0.0173, 0.99985]])  # half a turn and a degree
    S = np.eye(4, dtype=F)
    S[:3, :3] = F([[0, 0, 1], [-1, 0, 0], [0, -1, 0]])  # the camera looks along the robot's x
    S[:3, 3] = F([0.3, 0.0, 1.2])
    rig = Rig(hip_ctx, seqs, "f32", row_stride=2 * 18 * 66)
    cloud_rows = rig.run_cloud(sensor_in_robot=S)
    want = rig.check(2, 1, "far", rows=cloud_rows, sensor_in_robot=S)
    assert all(w["n_bad_rows"] == 0 and np.isfinite(w["row_normal"][:r["n"]]).all() for w, r in zip(want, cloud_rows))


def test_append_in_two_chunks_and_a_stride_exactly_full(hip_ctx):
    """two chunks of two frames of a sequence whose every pixel is valid: the second call leaves the first chunk's rows as they are,
    and fills row_stride to its last row"""
    frames, rows, cols = 2, 9, 66
    full = frames * rows * cols
    rig = Rig(hip_ctx, [sequence(_rng(9, b), frames, rows, cols, "f32") for b in range(2)], "f32", row_stride=2 * full)
    chunks = [[dict(depth=(2.0 + 0.3 * _rng(9, c, b).random((frames, rows, cols))).astype(F), n_images=None, pose=poses(_rng(9, c, b, 1), frames))
               for b in range(2)] for c in range(2)]
    rig.upload(chunks[0])
    first_rows = rig.run_cloud()
    first = rig.check(2, 1, "chunk 0", rows=first_rows)
    assert [r["n"] for r in first_rows] == [full, full]
    rig.upload(chunks[1])
    rig.run_cloud(append=True)
    second_rows = rig.host_rows(bases=[full, full])
    assert [r["n"] for r in second_rows] == [2 * full, 2 * full]
    import torch
    rig.nb.normal.view(torch.uint8).fill_(SENTINEL)
    rig.nb.n_normal.view(torch.uint8).fill_(SENTINEL)
    second = rig.check(2, 1, "chunk 1", rows=second_rows, append=True, before=dict(row_normal=[w["row_normal"] for w in first]))
    for a, b in zip(first, second):
        assert b["row_normal"][:full].tobytes() == a["row_normal"][:full].tobytes() and (b["row_normal"][full:, 3] > 0).any()
    assert rig.nb.n_rows.cpu().tolist() == [2 * full, 2 * full]


def test_a_skipped_frame_and_bad_rows(hip_ctx):
    import torch
    frames, rows, cols = 3, 9, 66
    seqs = [sequence(_rng(10, b), frames, rows, cols, "u16", pose_stride=4, index=True) for b in range(2)]
    seqs[0]["frame_index"][1] = 7                 # the cloud skips the frame: no row of it
    seqs[1]["pose"][seqs[1]["frame_index"][2], 6] = np.nan
    rig = Rig(hip_ctx, seqs, "u16", row_stride=frames * rows * cols)
    cloud_rows = rig.run_cloud()
    assert rig.cloud.n_skipped.cpu().tolist() == [1, 1]
    assert all(w["n_bad_rows"] == 0 for w in rig.check(2, 1, "skipped", rows=cloud_rows))
    assert 1 not in cloud_rows[0]["frame"][:cloud_rows[0]["n"]] and 2 not in cloud_rows[1]["frame"][:cloud_rows[1]["n"]]
    # rows that a caller got wrong: a frame or a pixel outside, a row of the skipped frame, one of the frame whose pose is not finite
    node, row = rig.cloud.node.cpu().numpy(), rig.cloud.row.cpu().numpy()
    node[0, [3, 4, 5]], row[0, [6, 7]] = [-1, frames, 1], [-1, rows * cols]
    node[1, [0, 300]] = 2
    rig.cloud.node.copy_(torch.from_numpy(node))
    rig.cloud.row.copy_(torch.from_numpy(row))
    want = rig.check(2, 1, "bad rows", rows=rig.host_rows())
    assert [w["n_bad_rows"] for w in want] == [5, 2]
    assert not want[0]["row_normal"][3:8].any() and not want[1]["row_normal"][[0, 300]].any()
    # n_images below frames: the rows of the images behind it are bad as well
    seqs[0]["n_images"], seqs[1]["n_images"] = 3, 1
    rig.upload(seqs)
    want = rig.check(2, 1, "rows of unserved images", rows=rig.host_rows())
    assert want[1]["n_bad_rows"] > 300 and (want[1]["normal"][1:].view(np.uint8) == SENTINEL).all()
    # a sequence whose row counts are out of range is refused whole
    for bases, n in (([0, 5], [10, 4]), ([0, -1], [10, 10]), ([0, 0], [10, frames * rows * cols + 1])):
        rig.cloud.n_out.copy_(torch.tensor(n, dtype=torch.int32))
        rig.nb.n_rows.copy_(torch.tensor(bases, dtype=torch.int32))
        rig.fill_sentinel()
        want = rig.check(2, 1, "refused rows", rows=rig.host_rows(bases), append=True, before={})
        assert [w["status"] for w in want] == [0, ref.PRS_ERR_RANGE]
        assert (want[1]["normal"].view(np.uint8) == SENTINEL).all() and (want[1]["row_normal"].view(np.uint8) == SENTINEL).all()
        assert want[1]["n_bad_rows"] is None


# ---- 5. determinism and capture ---------------------------------------------------------------------------------------------------------
def test_captured_graph_replayed_twice(hip_ctx):
    import torch
    ctx = hip_ctx
    frames, rows, cols = 2, 2 * TH + 1, TW + 9
    seqs = [sequence(_rng(11, b), frames, rows, cols, "f32", n_images=n) for b, n in enumerate((2, 1))]
    rig = Rig(ctx, seqs, "f32", row_stride=frames * rows * cols)
    cloud_rows = rig.run_cloud()
    eager = rig.check(2, 1, "eager", rows=cloud_rows)
    p, rp = rig.params(2, 1)
    i = rig.inputs()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        rig.nb.run(ctx, p, cloud=rig.cloud, **i)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rig.nb.run(ctx, p, cloud=rig.cloud, **i)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    torch.cuda.synchronize()
    for replay in range(2):
        rig.fill_sentinel()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        rig.compare(rig.outputs(), eager, "replay %d" % replay)
    # and on other images, a sequence of which is refused now
    rig.upload([sequence(_rng(11, b, 1), frames, rows, cols, "f32", n_images=n) for b, n in enumerate((1, 3))])
    cloud_rows = rig.run_cloud()
    rig.fill_sentinel()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    want = rig.expected(rp, cloud_rows)
    rig.compare(rig.outputs(), want, "replay on other images")
    assert [w["status"] for w in want] == [0, ref.PRS_ERR_RANGE]


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def test_call_level_refusals_write_nothing(hip_ctx):
    frames, rows, cols = 2, 9, 20
    seqs = [sequence(_rng(12, b), frames, rows, cols, "f32", n_images=frames, pose_stride=3, index=True) for b in range(2)]
    rig = Rig(hip_ctx, seqs, "f32", row_stride=frames * rows * cols)
    rig.run_cloud()
    lib, ctx = _lib_normals.load(), hip_ctx._h
    P = lambda **kw: ops.depth_normals_params(K, depth_type="f32", **kw)  # noqa: E731

    def D(rows=True):
        i = rig.inputs()
        return rig.nb.descriptor(P(), cloud=rig.cloud, **i) if rows else rig.nb.descriptor(P(), i["depth"], n_images=i["n_images"])

    def run(d, p=None):
        p = P() if p is None else p
        return lib.prs_depth_normals_batch_run(ctx, C.byref(p) if p != "null" else None, C.byref(d) if d is not None else None)

    rig.fill_sentinel()
    assert run(D()) == 0 and run(D(False)) == 0
    hip_ctx.synchronize()
    rig.fill_sentinel()
    row_pointers = ("row_frame", "row_pixel", "row_n", "row_normal", "n_bad_rows")
    # PRS_ERR_NULL: a struct or a required pointer unset, the row pointers set only in part
    assert run(None) == -1 and run(D(), "null") == -1
    for field in ("depth", "normal", "status", "pose") + row_pointers:
        d = D()
        setattr(d, field, None)
        assert run(d) == -1, field
    for field in row_pointers:
        d = D(False)
        setattr(d, field, getattr(D(), field))
        assert run(d) == -1, field
    d = D()
    for field in row_pointers:  # none of them: pose, frame_index and row_base alone ask for no rows
        setattr(d, field, None)
    assert run(d) == 0
    hip_ctx.synchronize()
    assert (rig.nb.row_normal.cpu().numpy().view(np.uint8) == SENTINEL).all()
    rig.fill_sentinel()
    # PRS_ERR_RANGE
    for field, value in (("batch", 0), ("frames", 0), ("rows", 0), ("cols", -1), ("pose_stride", 0), ("row_stride", 0), ("pitch", 76),
                         ("pitch", 82), ("pitch", -80)):
        d = D()
        setattr(d, field, value)
        assert run(d) == ref.PRS_ERR_RANGE, (field, value)
    nan, inf = float("nan"), float("inf")
    for field, value in (("radius", 0), ("radius", 9), ("radius", -1), ("smooth", -1), ("smooth", 4), ("max_rel_diff", -1.0),
                         ("max_rel_diff", nan), ("max_rel_diff", inf), ("depth_scaling_factor_to_meters", 0.0),
                         ("depth_scaling_factor_to_meters", -1.0), ("depth_scaling_factor_to_meters", nan), ("fx", inf), ("fy", nan),
                         ("cx", -inf), ("cy", nan), ("range_min", -1.0), ("range_min", 11.0), ("range_min", nan), ("range_max", inf)):
        p = P()
        setattr(p, field, value)
        assert run(D(), p) == ref.PRS_ERR_RANGE, (field, value)
        assert run(D(False), p) == ref.PRS_ERR_RANGE, (field, value)
    p = P()
    p.sensor_in_robot[14] = nan
    assert run(D(), p) == ref.PRS_ERR_RANGE
    # PRS_ERR_UNSUPPORTED
    for value in (2, -1):
        p = P()
        p.depth_type = value
        assert run(D(), p) == -5, value
    for field, step in (("depth", 2), ("normal", 8), ("normal", 4), ("row_normal", 8), ("n_images", 2), ("pose", 2), ("frame_index", 1),
                        ("row_frame", 2), ("row_pixel", 1), ("row_n", 2), ("n_normal", 2), ("n_bad_rows", 1), ("status", 2)):
        d = D()
        setattr(d, field, getattr(d, field) + step)
        assert run(d) == -5, field
    d = D()
    d.row_base = d.row_n + 2
    assert run(d) == -5
    # more pixels than 2^31 - 1, and more workgroups than one launch takes (2^25 tiles of a pixel each)
    for b, f, r, c in ((1, 1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 15, 1, 1), (1, 1, 1 << 16, 1 << 15), (1 << 13, 1 << 12, 1, 1)):
        d = D(False)
        d.batch, d.frames, d.rows, d.cols, d.pitch = b, f, r, c, 4 * c
        assert run(d) == -5, (b, f, r, c)
    hip_ctx.synchronize()
    for k, v in rig.outputs().items():
        assert (v.view(np.uint8) == SENTINEL).all(), k
    assert b"prs_depth_normals_batch_run" in _lib_normals.load().prs_last_error(ctx)


def test_the_python_layer_refuses_what_it_cannot_describe(hip_ctx):
    import torch
    nb = ops.DepthNormalsBatch(2, 2, 5, 6, row_stride=60)
    p = ops.depth_normals_params(K, depth_type="f32")
    ok = torch.zeros((2, 2, 5, 6), dtype=torch.float32, device="cuda")
    pose = torch.zeros((2, 2, 16), dtype=torch.float32, device="cuda")
    cloud = ops.DepthCloudBatch(2, 2, 5, 6, 60)
    nb.descriptor(p, ok)
    nb.descriptor(p, ok, pose, cloud=cloud)
    for bad in (ok.to(torch.float64), ok[..., :5], ok[:, :, :4], ok.transpose(2, 3).contiguous().transpose(2, 3), ok[:, :1].expand(2, 2, 5, 6),
                torch.zeros((2, 2, 5, 6), dtype=torch.uint16, device="cuda")):
        with pytest.raises(ValueError):
            nb.descriptor(p, bad)
    with pytest.raises(ValueError):
        nb.descriptor(ops.depth_normals_params(K, depth_type="u16"), ok)
    for bad in (None, pose[:1], pose[..., :12], pose.reshape(2, 2, 4, 4), pose.to(torch.float64)):
        with pytest.raises(ValueError):
            nb.descriptor(p, ok, bad, cloud=cloud)
    with pytest.raises(ValueError):
        nb.descriptor(p, ok, n_images=torch.zeros((3,), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        nb.descriptor(p, ok, pose, frame_index=torch.zeros((2, 3), dtype=torch.int32, device="cuda"), cloud=cloud)
    with pytest.raises(ValueError):
        nb.descriptor(p, ok, append=True)  # nothing to append to
    for other in (ops.DepthCloudBatch(2, 2, 5, 6, 59), ops.DepthCloudBatch(2, 2, 6, 5, 60), ops.DepthCloudBatch(1, 2, 5, 6, 60),
                  ops.DepthCloudBatch(2, 2, 5, 6, 60, outputs=("frame",))):
        with pytest.raises(ValueError):
            nb.descriptor(p, ok, pose, cloud=other)
    with pytest.raises(ValueError):
        ops.DepthNormalsBatch(2, 2, 5, 6).descriptor(p, ok, pose, cloud=cloud)
    with pytest.raises(ValueError):
        ops.DepthNormalsBatch(2, 2, 5, 6).rows_of(torch.zeros((2, 3), dtype=torch.int32, device="cuda"))
    for bad in (torch.zeros((3, 3), dtype=torch.int32, device="cuda"), torch.zeros((2, 3), dtype=torch.float32, device="cuda"),
                torch.zeros((6,), dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError):
            nb.rows_of(bad)
    for bad in (dict(outputs=("normals",)), dict(rows=0), dict(batch=0), dict(row_stride=0), dict(batch=1 << 16, frames=1 << 15)):
        with pytest.raises(ValueError):
            ops.DepthNormalsBatch(**dict(dict(batch=1, frames=1, rows=2, cols=2), **bad))


def test_rows_of_gathers_on_the_device(hip_ctx):
    import torch
    nb = ops.DepthNormalsBatch(2, 1, 2, 3, row_stride=6)
    nb.row_normal.copy_(torch.arange(48, dtype=torch.float32).reshape(2, 6, 4))
    index = torch.tensor([[5, 0, 0, -1], [2, 6, 3, 1]], dtype=torch.int32, device="cuda")
    got = nb.rows_of(index)
    assert got.is_cuda and got.shape == (2, 4, 4)
    want = np.arange(48, dtype=F).reshape(2, 6, 4)
    assert np.array_equal(got.cpu().numpy(), np.stack([np.stack([want[0, 5], want[0, 0], want[0, 0], np.zeros(4, F)]),
                                                       np.stack([want[1, 2], np.zeros(4, F), want[1, 3], want[1, 1]])]))


# ---- 7. the chain -------------------------------------------------------------------------------------------------------------------------
def test_sgm_stereo_speckle_consistency_cloud_normals_voxel_ply(hip_ctx, tmp_path):
    """the chain of tests/test_depth_consistency_gpu.py at its shape, carried on: the cloud of the filtered depth, the normals of the
    same images with one per cloud row, the voxel filter over the cloud, its index gathering the normals, and a PLY with nx ny nz.
    Everything equals the restatements chained on the CPU"""
    import torch

    import test_depth_consistency_ref as ccases
    import depth_consistency_ref as cref
    import sgm_stereo_ref as sref
    import speckle_ref as fref
    import world_voxel_ref as vref
    from srrg2_proslam_amd import formats
    cam = dict(fx=40.0, fy=40.0, cx=30.0, cy=8.0, baseline_m=0.5)  # bf 20: a disparity of 4 is 5 m
    kw = dict(n_disparities=16, min_disparity=0, p1=10, p2=120, n_paths=8, uniqueness_percent=3, lr_max_diff=1)
    B, frames, rows, cols = 1, 3, 21, 70
    rng = _rng(11)
    right = rng.integers(0, 256, (B, frames, rows, cols), dtype=np.uint8)
    left = right[..., np.clip(np.arange(cols) - 4, 0, cols - 1)].copy()
    redraw = rng.random(left.shape) < 0.1
    left[redraw] = rng.integers(0, 256, int(redraw.sum()), dtype=np.uint8)
    pose = np.stack([ccases.at(0.002 * i, 0.0, 0.001 * i) for i in range(frames)])[None]
    ckw = dict(range_min=0.1, range_max=10.0, scale=1.0)
    fkw = dict(window=2, stride=1, max_rel_diff=0.05, min_support=2, max_violation=0)
    nkw = dict(radius=2, smooth=1, max_rel_diff=0.05)
    voxel = 0.25

    stereo = sref.sgm_stereo(left[0], right[0], None, sref.params(20.0, **kw))
    disparity = np.stack([i["disparity"] for i in stereo["results"]])
    depth = np.stack([i["depth"] for i in stereo["results"]])
    speckled = fref.speckle(disparity, depth, None, fref.params(4, 1.0))
    speckled_depth = np.stack([i["companion"] for i in speckled["results"]])
    filtered = cref.depth_consistency(dict(depth=speckled_depth, pose=pose[0]), cref.params(cam, **fkw, **ckw))
    want_depth = np.stack([i["out"] for i in filtered["results"]])
    stride = frames * rows * cols
    seq = dict(depth=want_depth, n_images=frames, pose=pose[0])
    want_cloud = cloud_ref.depth_cloud(seq, cloud_ref.params(cam, **ckw), stride)
    n = want_cloud["n_out"]
    want_normals = ref.depth_normals(seq, ref.params(cam, **nkw, **ckw), None,
                                     dict(frame=want_cloud["frame"], pixel=want_cloud["pixel"], n=n, base=None))
    want_voxel = vref.world_voxel(dict(in_stride=stride, n=n, xyz=want_cloud["xyz"], node=want_cloud["frame"], row=want_cloud["pixel"]),
                                  vref.params(voxel), stride)
    m = want_voxel["n_out"]
    want_rows = want_normals["row_normal"][want_voxel["index"]]
    assert 100 < m < n and (want_rows[:, 3] > 0).sum() > 50

    dev = torch.device("cuda", 0)
    ds = ops.SgmStereoBatch(B, frames, rows, cols)
    ds.run(hip_ctx, ops.sgm_stereo_params(cam, **kw), torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev))
    sf = ops.SpeckleFilterBatch(B, frames, rows, cols)
    sf.run(hip_ctx, ops.speckle_params(4, 1.0), ds.disparity, ds.depth)
    t_pose = torch.from_numpy(pose).to(dev)
    dcb = ops.DepthConsistencyBatch(B, frames, rows, cols, 2, "f32")
    out = dcb.run(hip_ctx, ops.depth_consistency_params(cam, depth_type="f32", **fkw, **ckw), ds.depth, t_pose)
    n_images = torch.tensor([frames], dtype=torch.int32, device=dev)
    dc = ops.DepthCloudBatch(B, frames, rows, cols, stride)
    dc.run(hip_ctx, ops.depth_cloud_params(cam, depth_type="f32", **ckw), out, t_pose, n_images)
    nb = ops.DepthNormalsBatch(B, frames, rows, cols, row_stride=stride)
    nb.run(hip_ctx, ops.depth_normals_params(cam, depth_type="f32", **nkw, **ckw), out, t_pose, n_images, cloud=dc)
    wv = ops.WorldVoxelBatch(B, stride, stride)
    wv.run(hip_ctx, ops.world_voxel_params(voxel), dc)
    fused_normals = nb.rows_of(wv.index)
    hip_ctx.synchronize()
    assert out.cpu().numpy().tobytes() == want_depth[None].tobytes()
    assert nb.status.cpu().tolist() == [0] and nb.n_bad_rows.cpu().tolist() == [0]
    assert nb.normal.cpu().numpy().tobytes() == want_normals["normal"][None].tobytes()
    assert nb.n_normal.cpu().numpy().tolist() == [want_normals["n_normal"].tolist()]
    assert nb.row_normal.cpu().numpy()[0, :n].tobytes() == want_normals["row_normal"][:n].tobytes()
    fused = wv.cloud_of(0)
    assert fused["n_out"] == m and fused["index"].tobytes() == want_voxel["index"].tobytes()
    got_rows = fused_normals.cpu().numpy()[0, :m]
    assert got_rows.tobytes() == want_rows.tobytes()
    got_ply, want_ply = str(tmp_path / "got.ply"), str(tmp_path / "want.ply")
    formats.write_ply(got_ply, fused["xyz"], normals=got_rows)
    formats.write_ply(want_ply, want_voxel["xyz"], normals=want_rows)
    written = open(got_ply, "rb").read()
    assert written == open(want_ply, "rb").read() and b"property float nz" in written and len(written.split(b"end_header\n", 1)[1]) == 24 * m
