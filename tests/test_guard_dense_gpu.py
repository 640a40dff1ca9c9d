"""Every dense image stage inside guard bands (tests/guarded.py) at the buffer sizes and alignments include/proslam_hip.h documents.

Each case builds its inputs and its expected result with the builders and the restatement of the stage's own GPU test, moves every
caller-owned array of the call into an arena -- at exactly the demanded alignment, with a band of fill bytes on either side, the
workspace exactly as large as prs_*_workspace_bytes answers for the parameters of this very run -- and runs twice, with fill 0x00
and with fill 0xFF.  Both runs must equal the restatement as the stage's own test asserts it, equal each other byte for byte, and
leave every band clean.  The stage tests' SENTINEL is set to the fill, so output elements a call must not touch (pitch padding,
rows from the count to the stride, images from n_images to frames) are fill before the call and asserted to be fill after it.
The last sequence of a batch is always the full one, so its last image, row or pixel adjoins a band."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded
import test_dense_stereo_gpu as stereo
import test_depth_cloud_gpu as cloud
import test_depth_consistency_gpu as consistency
import test_rectify_gpu as rectify
import test_rgbd_gpu as rgbd
import test_sgm_stereo_gpu as sgm
import test_speckle_gpu as speckle
from srrg2_proslam_amd import _lib, ops

pytestmark = pytest.mark.gpu
F = np.float32
B, FRAMES, ROWS, COLS = 2, 2, 33, 65     # scalar tails everywhere: no pitch is a multiple of four elements
VROWS, VCOLS = 16, 64                    # the shape of the vector paths
N_IMAGES = (1, 2)                        # the last sequence is the full one


def lib():
    return _lib.load()


def slack_images(host, n_images, fill):
    """the images from n_images[b] to frames of a host array [B, frames, ...] become fill bytes: the contract says they are not read"""
    for b, n in enumerate(n_images):
        host[b, n:] = guarded.host_fill(host.dtype, fill)
    return host


# ---- rectifier ------------------------------------------------------------------------------------------------------------------------
# (pixel, interpolation, src shape, dst shape, src pitch in elements, src alignment, dst pitch in elements, dst alignment).  dst is
# 4-byte aligned by contract; a lane's four pixels go out in one store when dst and dst_pitch are multiples of four elements
RECTIFY = {
    "u8_33x65": ("u8", "bilinear", (33, 65), None, 65, 1, 65, 4),            # scalar taps from global memory, scalar stores
    "u8_to_17x40": ("u8", "bilinear", (33, 65), (17, 40), 65, 1, 40, 4),
    "u8_staged_pitch80_dst64": ("u8", "bilinear", (33, 65), (33, 64), 80, 16, 64, 4),  # stage_ok and one 4-byte store a lane
    "u8_dst65_pitch68": ("u8", "bilinear", (33, 65), None, 65, 1, 68, 4),     # vector stores and a scalar tail in every row
    "u16_nearest_9x13": ("u16", "nearest", (9, 13), None, 13, 2, 14, 4),
    "u16_nearest_9x13_vector": ("u16", "nearest", (9, 13), None, 13, 2, 16, 8),
    "f32_nearest_9x13": ("f32", "nearest", (9, 13), None, 13, 4, 13, 4),
    "f32_nearest_9x13_vector": ("f32", "nearest", (9, 13), None, 13, 4, 16, 16),
}
NP_PIXEL = dict(u8=np.uint8, u16=np.uint16, f32=np.float32)


@pytest.mark.parametrize("name", sorted(RECTIFY))
def test_rectifier(hip_ctx, name):
    pixel, interpolation, src_shape, dst_shape, sp, src_align, dp, dst_align = RECTIFY[name]
    np_dtype = NP_PIXEL[pixel]
    es = np.dtype(np_dtype).itemsize
    rows, cols = src_shape
    drows, dcols = dst_shape or src_shape
    n = 3
    src = rectify.image(np.random.default_rng([7, rows, cols, es]), src_shape, np_dtype, batch=n)
    maps = [rectify.make_map("euroc", src_shape, dst_shape), rectify.make_map("wide", src_shape, dst_shape)]
    map_of = [1, 0, 1]
    border = 9
    want, want_border, want_status = rectify.ref.rectify_batch(src, maps, map_of, dst_shape, interpolation, border)
    params = ops.rectify_params(pixel, interpolation, border)
    arr = (_lib.RectifyMap * len(maps))(*[m.struct() for m in maps])
    tdtype = {np.uint8: torch.uint8, np.uint16: torch.uint16, np.float32: torch.float32}[np_dtype]

    def case(arena):
        # staging reads whole 16-byte pieces of a source row, so there the last row has up16(cols) bytes (the header says so)
        staged = src_align == 16 and (sp * es) % 16 == 0
        last = (cols * es + 15) // 16 * 16 if staged else cols * es
        t_src = arena.take((n, rows, sp), tdtype, src_align, "src", extent=((n * rows - 1) * sp) * es + last)
        t_src[..., :cols].copy_(torch.from_numpy(src))
        t_dst = arena.take((n, drows, dp), tdtype, dst_align, "dst", extent=((n * drows - 1) * dp + dcols) * es)
        t_maps = arena.take((C.sizeof(arr),), torch.uint8, 4, "maps")
        t_maps.copy_(torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()))
        t_map_of = arena.take((n,), torch.int32, 4, "map_of")
        t_map_of.copy_(torch.tensor(map_of, dtype=torch.int32))
        t_border, t_status = arena.take((n,), torch.int32, 4, "n_border"), arena.take((n,), torch.int32, 4, "status")
        d = _lib.RectifyBatch()
        d.batch, d.src_rows, d.src_cols, d.src_pitch, d.src = n, rows, cols, sp * es, t_src.data_ptr()
        d.dst_rows, d.dst_cols, d.dst_pitch, d.dst = drows, dcols, dp * es, t_dst.data_ptr()
        d.n_maps, d.maps, d.map_of = len(maps), t_maps.data_ptr(), t_map_of.data_ptr()
        d.n_border, d.status = t_border.data_ptr(), t_status.data_ptr()
        assert lib().prs_rectify_batch_run(hip_ctx._h, C.byref(params), C.byref(d)) == 0
        hip_ctx.synchronize()
        out = dict(dst=t_dst.cpu().numpy(), n_border=t_border.cpu().numpy(), status=t_status.cpu().numpy())
        assert rectify.same_bits(np.ascontiguousarray(out["dst"][..., :dcols]), want), name
        assert (out["dst"][..., dcols:].view(np.uint8) == arena.fill).all(), "bytes between dst_cols and dst_pitch were written"
        assert np.array_equal(out["n_border"], want_border) and np.array_equal(out["status"], want_status)
        return out

    guarded.both_fills(case)
    assert (want_border > 0).any() and (want_border < drows * dcols).all()


# ---- RGB-D measurements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("np_dtype", [np.uint16, np.float32], ids=["u16", "f32"])
def test_rgbd_measurements(hip_ctx, np_dtype):
    """three frames of 33 x 65 depth pixels with 17, 40 and 301 = capacity keypoints: the last frame's last keypoint, descriptor and
    intensity adjoin the bands, and so does the last compacted measurement whenever every keypoint has a depth"""
    rng = np.random.default_rng([8, np.dtype(np_dtype).itemsize])
    stride, counts, n = 301, (17, 40, 301), 3
    depth = rng.integers(1, 9000, (n, ROWS, COLS)).astype(np_dtype) if np_dtype == np.uint16 else rng.uniform(0.2, 9.0, (n, ROWS, COLS)).astype(F)
    depth[:2][rng.random((2, ROWS, COLS)) < 0.2] = 0                        # the last frame keeps all 301: its outputs end at the band
    kps = [np.stack([rng.uniform(-0.49, COLS - 0.51, k), rng.uniform(-0.49, ROWS - 0.51, k)], axis=1).astype(F) for k in counts]
    kps[2][-1] = (COLS - 1, ROWS - 1)                                      # the last keypoint reads the last pixel of the last image
    scale = 1e-3 if np_dtype == np.uint16 else 1.0
    desc = rng.integers(0, 256, (n, stride, 32), dtype=np.uint8)
    inten = rng.uniform(0, 255, (n, stride)).astype(F)
    tdtype = torch.uint16 if np_dtype == np.uint16 else torch.float32

    def case(arena):
        kp = np.full((n, stride, 2), guarded.host_fill(F, arena.fill), F)
        h_desc, h_inten = desc.copy(), inten.copy()
        for b, k in enumerate(kps):
            kp[b, :len(k)] = k
            h_desc[b, len(k):] = arena.fill
            h_inten[b, len(k):] = guarded.host_fill(F, arena.fill)
        t = {}
        for name, host, dt, align in (("depth", depth, tdtype, depth.itemsize), ("keypoints", kp, torch.float32, 8),
                                      ("descriptors", h_desc, torch.uint8, 16), ("intensity", h_inten, torch.float32, 4),
                                      ("n_features", np.array(counts, np.int32), torch.int32, 4)):
            t[name] = arena.take(host.shape, dt, align, name)
            t[name].copy_(torch.from_numpy(host))
        t["fixed"] = arena.take((n, stride, 4), torch.float32, 16, "fixed")
        t["fixed_desc"] = arena.take((n, stride, 32), torch.uint8, 16, "fixed_desc")
        t["fixed_intensity"] = arena.take((n, stride), torch.float32, 4, "fixed_intensity")
        t["n_fixed"], t["status"] = arena.take((n,), torch.int32, 4, "n_fixed"), arena.take((n,), torch.int32, 4, "status")
        ops.depth_measurements_batch(hip_ctx, ops.depth_params("u16" if np_dtype == np.uint16 else "f32", scale), t["depth"], t["keypoints"],
                                     t["descriptors"], t["n_features"], t["fixed"], t["fixed_desc"], t["n_fixed"], t["status"], t["intensity"],
                                     t["fixed_intensity"])
        hip_ctx.synchronize()
        out = dict(fixed=t["fixed"].cpu().numpy(), desc=t["fixed_desc"].cpu().numpy(), inten=t["fixed_intensity"].cpu().numpy(),
                   n_fixed=t["n_fixed"].cpu().numpy(), status=t["status"].cpu().numpy())
        inp = dict(depth=depth, kp=kp, desc=h_desc, inten=h_inten, n=list(counts), stride=stride, es=None, scale=scale)
        for b in range(n):
            assert rgbd._same(inp, out, b) >= 0
            k = int(out["n_fixed"][b])
            for name in ("fixed", "desc", "inten"):  # rows from the count to the stride are not written
                assert (np.ascontiguousarray(out[name][b, k:]).view(np.uint8) == arena.fill).all(), (b, name)
        assert int(out["n_fixed"][2]) == stride
        return out

    guarded.both_fills(case)


# ---- depth cloud ----------------------------------------------------------------------------------------------------------------------
def cloud_case(hip_ctx, monkeypatch, depth_type, step, shape=(ROWS, COLS), short=0, bases=None, understate=None, depth_align=None):
    """-> case(arena) for guarded.both_fills.  out_stride = the restatement's n_total of the last, full sequence less `short`;
    understate: a name of the arena's records whose extent the harness is told 16 bytes (one row) short"""
    rows, cols = shape
    seqs = [cloud.sequence(cloud._rng(21, rows, cols, b), FRAMES, rows, cols, depth_type, n_images=N_IMAGES[b], gray=True, index=True)
            for b in range(B)]
    scale = 1e-3 if depth_type == "u16" else 1.0
    rp = cloud.ref.params(cloud.K, step=step, scale=scale)
    totals = [cloud.ref.depth_cloud(dict(s, n_base=None if bases is None else bases[b]), rp, 0 if bases is None else bases[b],
                                    count_only=True)["n_total"] for b, s in enumerate(seqs)]
    out_stride = totals[-1] - short
    assert totals[-1] == max(totals) and out_stride > 0

    def case(arena):
        monkeypatch.setattr(cloud, "SENTINEL", arena.fill)
        for s in seqs:
            slack_images(s["depth"][None], [s["n_images"]], arena.fill)
            slack_images(s["gray"][None], [s["n_images"]], arena.fill)
        rig = cloud.Rig(hip_ctx, seqs, out_stride, depth_type)
        arena.adopt(rig.t, "depth", depth_align or (2 if depth_type == "u16" else 4))
        arena.adopt(rig.t, "gray", 1)
        for name in ("pose", "n_images", "frame_index"):
            arena.adopt(rig.t, name, 4)
        arena.adopt(rig.dc, "xyz", 16, extent=(B * out_stride - 1) * 16 if understate == "xyz" else None)
        for name in ("node", "row", "n_out", "n_total", "n_skipped", "status"):
            arena.adopt(rig.dc, name, 4)
        arena.workspace(rig.dc, lib().prs_depth_cloud_workspace_bytes(B, FRAMES, rows, cols, step))
        want = rig.check("guarded", bases=bases, step=step)
        assert want[-1]["n_total"] == totals[-1] and want[-1]["n_out"] == out_stride
        assert want[-1]["status"] == (cloud.ref.PRS_ERR_CAPACITY if short else cloud.ref.PRS_OK)
        assert want[0]["n_out"] < out_stride  # the first sequence leaves rows from its count to the stride
        return arena, rig.outputs()

    return case


def outputs_only(case):
    return lambda arena: case(arena)[1]


@pytest.mark.parametrize("short", [0, 1], ids=["exact", "one_short"])
@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("depth_type", ["u16", "f32"])
def test_depth_cloud(hip_ctx, monkeypatch, depth_type, step, short):
    guarded.both_fills(outputs_only(cloud_case(hip_ctx, monkeypatch, depth_type, step, short=short)))


@pytest.mark.parametrize("vector", [False, True], ids=["element_aligned", "load_aligned"])
@pytest.mark.parametrize("depth_type", ["u16", "f32"])
def test_depth_cloud_vector_loads(hip_ctx, monkeypatch, depth_type, vector):
    """16 x 64 at step 1: a lane reads its four depths in one load when the array is aligned to that load (8 bytes of 16-bit depths, 16
    of floats) and runs the scalar path, at the same shape, when it is aligned to its element alone"""
    align = (8 if depth_type == "u16" else 16) if vector else None
    guarded.both_fills(outputs_only(cloud_case(hip_ctx, monkeypatch, depth_type, 1, shape=(VROWS, VCOLS), depth_align=align)))


def test_depth_cloud_appends_behind_n_base(hip_ctx, monkeypatch):
    guarded.both_fills(outputs_only(cloud_case(hip_ctx, monkeypatch, "u16", 1, bases=[7, 11])))


# ---- dense stereo and SGM -------------------------------------------------------------------------------------------------------------
def stereo_case(hip_ctx, monkeypatch, mod, shape, kw, workspace_bytes, rig_kw=None, understate_workspace=0):
    rows, cols = shape
    left, right = mod.pairs(mod._rng(31, rows, cols), (B, FRAMES, rows, cols), shift=12)

    def case(arena):
        monkeypatch.setattr(mod, "SENTINEL", arena.fill)
        l, r = slack_images(left.copy(), N_IMAGES, arena.fill), slack_images(right.copy(), N_IMAGES, arena.fill)
        rig = mod.Rig(hip_ctx, l, r, list(N_IMAGES), **(rig_kw or {}))
        arena.adopt(rig.images, 0, 1, name="left")
        arena.adopt(rig.images, 1, 1, name="right")
        arena.adopt(rig, "t_n", 4, name="n_images")
        for name in ("_disparity", "_depth"):
            arena.adopt_pitched(rig.ds, name, cols, 4)
        rig.ds.disparity, rig.ds.depth = rig.ds._disparity[..., :cols], rig.ds._depth[..., :cols]
        arena.adopt(rig.ds, "n_valid", 4)
        arena.adopt(rig.ds, "status", 4)
        nbytes = int(workspace_bytes)
        assert nbytes > 0
        rig.ds.workspace = arena.take((nbytes,), torch.uint8, 16, "workspace", extent=nbytes - understate_workspace)
        results = rig.check("guarded", **kw)
        valid = mod.n_valid(results)
        assert len(valid) == sum(N_IMAGES) and (rows * cols < 1000 or kw["n_disparities"] == 1 or min(valid) > 0)
        return arena, rig.outputs()

    return case


DENSE = {
    "r0_lr": dict(shape=(ROWS, COLS), aggregation_radius=0, lr_max_diff=1),
    "r7_lr": dict(shape=(ROWS, COLS), aggregation_radius=7, lr_max_diff=2),
    "r0_no_lr": dict(shape=(ROWS, COLS), aggregation_radius=0, lr_max_diff=-1),
    "r7_no_lr": dict(shape=(ROWS, COLS), aggregation_radius=7, lr_max_diff=-1),
    "16x64_r3_lr": dict(shape=(VROWS, VCOLS), aggregation_radius=3, lr_max_diff=1),
}


@pytest.mark.parametrize("name", sorted(DENSE))
def test_dense_stereo(hip_ctx, monkeypatch, name):
    """37 disparities from 7; the workspace is asked with lr_check = 0 exactly when lr_max_diff is -1"""
    kw = dict(DENSE[name], n_disparities=37, min_disparity=7)
    rows, cols = kw.pop("shape")
    nbytes = lib().prs_dense_stereo_workspace_bytes(B, FRAMES, rows, cols, 37, int(kw["lr_max_diff"] >= 0))
    assert (kw["lr_max_diff"] >= 0) == (nbytes == lib().prs_dense_stereo_workspace_bytes(B, FRAMES, rows, cols, 37, 1))
    guarded.both_fills(outputs_only(stereo_case(hip_ctx, monkeypatch, stereo, (rows, cols), kw, nbytes)))


# n_disparities, n_paths, images_in_flight (of four images), lr_max_diff
SGM = {
    "d1_p4_f3": dict(shape=(ROWS, COLS), n_disparities=1, n_paths=4, in_flight=3, lr_max_diff=1),
    "d37_p8_f1": dict(shape=(ROWS, COLS), n_disparities=37, n_paths=8, in_flight=1, lr_max_diff=1),
    "d37_p4_f3_no_lr": dict(shape=(ROWS, COLS), n_disparities=37, n_paths=4, in_flight=3, lr_max_diff=-1),
    "d64_p8_f3": dict(shape=(ROWS, COLS), n_disparities=64, n_paths=8, in_flight=3, lr_max_diff=1),
    "16x64_d64_p4_f1": dict(shape=(VROWS, VCOLS), n_disparities=64, n_paths=4, in_flight=1, lr_max_diff=0),
}


def sgm_case(hip_ctx, monkeypatch, name, understate_workspace=0):
    kw = dict(SGM[name], min_disparity=7 if SGM[name]["n_disparities"] > 1 else 12)
    rows, cols = kw.pop("shape")
    in_flight = kw.pop("in_flight")
    nbytes = lib().prs_sgm_stereo_workspace_bytes(B, FRAMES, rows, cols, kw["n_disparities"], int(kw["lr_max_diff"] >= 0), in_flight)
    assert nbytes < lib().prs_sgm_stereo_workspace_bytes(B, FRAMES, rows, cols, 256, 1, B * FRAMES)  # not what ops.py asks for
    return stereo_case(hip_ctx, monkeypatch, sgm, (rows, cols), kw, nbytes, dict(images_in_flight=in_flight, n_disparities=kw["n_disparities"]),
                       understate_workspace)


@pytest.mark.parametrize("name", sorted(SGM))
def test_sgm_stereo(hip_ctx, monkeypatch, name):
    guarded.both_fills(outputs_only(sgm_case(hip_ctx, monkeypatch, name)))


# ---- speckle filter -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(ROWS, COLS), (VROWS, VCOLS)], ids=["33x65", "16x64"])
@pytest.mark.parametrize("kinds", [(np.float32, np.float32), (np.uint16, np.float32), (np.float32, np.uint16), (np.uint16, None)],
                         ids=["f32_f32", "u16_f32", "f32_u16", "u16_alone"])
def test_speckle(hip_ctx, monkeypatch, kinds, shape):
    rows, cols = shape
    rng = speckle._rng(41, rows, cols)
    images = speckle.noise(rng, (B, FRAMES, rows, cols), 0.62, dtype=kinds[0])
    companions = None if kinds[1] is None else rng.integers(1, 1000, images.shape).astype(kinds[1])

    def case(arena):
        monkeypatch.setattr(speckle, "SENTINEL", arena.fill)
        im = slack_images(images.copy(), N_IMAGES, arena.fill)
        co = None if companions is None else slack_images(companions.copy(), N_IMAGES, arena.fill)
        rig = speckle.Rig(hip_ctx, im, co, list(N_IMAGES))
        arena.adopt(rig, "t_image", im.itemsize, name="image")
        if co is not None:
            arena.adopt(rig, "t_companion", co.itemsize, name="companion")
        arena.adopt(rig, "t_n", 4, name="n_images")
        arena.adopt_pitched(rig.sf, "_label", cols, 4)
        rig.sf.label = rig.sf._label[..., :cols]
        for name in ("n_kept", "n_removed", "status"):
            arena.adopt(rig.sf, name, 4)
        arena.workspace(rig.sf, lib().prs_speckle_workspace_bytes(B, FRAMES, rows, cols))
        results = rig.check(4, 1.0, "guarded")
        assert all(i["n_kept"] > 0 and i["n_removed"] > 0 for i in speckle.images_of(results))
        return rig.outputs()

    guarded.both_fills(case)


# ---- depth consistency ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 3])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["u16", "f32"])
def test_depth_consistency(hip_ctx, monkeypatch, dtype, window):
    """five frames, the workspace for exactly this window, every optional output on"""
    frames, n_images = 5, (3, 5)
    depth, pose, camera = consistency.sequences(consistency._rng(51, window), B, frames, ROWS, COLS, dtype, poses=frames)
    index = np.stack([np.random.default_rng([52, b]).permutation(frames).astype(np.int32) for b in range(B)])

    def case(arena):
        monkeypatch.setattr(consistency, "SENTINEL", arena.fill)
        d = slack_images(depth.copy(), n_images, arena.fill)
        idx = index.copy()
        for b, n in enumerate(n_images):
            idx[b, n:] = -1 if arena.fill else 0
        rig = consistency.Rig(hip_ctx, d, pose, list(n_images), idx, window=window, outputs=consistency.OUTPUTS)
        arena.adopt(rig, "t_depth", d.itemsize, name="depth")
        for name in ("t_pose", "t_n", "t_index"):
            arena.adopt(rig, name, 4, name=name[2:])
        arena.adopt_pitched(rig.dcb, "_out", COLS, d.itemsize)
        arena.adopt_pitched(rig.dcb, "_support", COLS, 1)
        arena.adopt_pitched(rig.dcb, "_violation", COLS, 1)
        rig.dcb.out, rig.dcb.support, rig.dcb.violation = (t[..., :COLS] for t in (rig.dcb._out, rig.dcb._support, rig.dcb._violation))
        for name in ("n_kept", "n_removed", "n_skipped", "status"):
            arena.adopt(rig.dcb, name, 4)
        arena.workspace(rig.dcb, lib().prs_depth_consistency_workspace_bytes(B, frames, window))
        results = rig.check(camera, "guarded", window=window, min_support=1)
        images = consistency.images_of(results)
        assert len(images) == sum(n_images) and all(i["n_kept"] > 0 and i["n_removed"] > 0 for i in images)
        return rig.outputs()

    guarded.both_fills(case)


# ---- the check bites: the harness is told an extent one element short, the kernel the truth --------------------------------------------
def test_an_understated_xyz_extent_is_reported(hip_ctx, monkeypatch):
    """the cloud's last compacted row, at out_stride == n_total, lies where the harness believes the trailing band to begin"""
    arena, _ = cloud_case(hip_ctx, monkeypatch, "u16", 1, understate="xyz")(guarded.Arena(0xFF))
    bad = arena.violations()
    assert bad and {(name, side) for name, side, _ in bad} == {("xyz", "after")} and min(o for _, _, o in bad) == 0 and max(o for _, _, o in bad) < 16


def test_an_understated_sgm_workspace_is_reported(hip_ctx, monkeypatch):
    """the workspace's last 16 bytes: the end of the S volume, which the last image's last pixels are written to"""
    arena, _ = sgm_case(hip_ctx, monkeypatch, "d37_p8_f1", understate_workspace=16)(guarded.Arena(0xFF))
    bad = arena.violations()
    assert bad and {(name, side) for name, side, _ in bad} == {("workspace", "after")} and min(o for _, _, o in bad) == 0 and max(o for _, _, o in bad) < 16
