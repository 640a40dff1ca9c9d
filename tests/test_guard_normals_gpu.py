"""prs_depth_normals_batch_run inside guard bands (tests/guarded.py) at the buffer sizes and alignments
include/proslam_hip_normals.h documents, with and without cloud rows.

Every caller-owned array of the call lies in an arena, at exactly the demanded alignment (a multiple of it, never of twice it), with a
band of fill bytes on either side and not one byte more than the header gives it: depth ends with the last pixel of the last row of
the last image, not with that row's pitch.  A case runs with fill 0x00 and with fill 0xFF; both runs must equal the restatement,
equal each other byte for byte and leave every band clean.  What the call must not read -- the images from n_images on, the cloud
rows from row_n on -- holds the fill (NaN or 65535 as a depth, -1 as a frame), what it must not write is fill before and after.
The last sequence is the full one, so its last image and row adjoin a band.  One case understates an extent on purpose, to show that
the harness reports a write behind it."""
import ctypes as C

import numpy as np
import pytest
import torch

import depth_cloud_ref as cloud_ref
import depth_normals_cases as cases
import depth_normals_ref as ref
import guarded
from srrg2_proslam_amd import _lib_normals, ops

pytestmark = pytest.mark.gpu
F = np.float32
B, FRAMES, ROWS, COLS = 2, 2, 33, 65   # ragged tiles; no pitch is a multiple of four elements
N_IMAGES = (1, 2)                      # the last sequence is the full one
K = cases.K


def filled(shape, dtype, fill):
    return np.full(shape, guarded.host_fill(dtype, fill), dtype)


def build(depth_type, with_rows, seed=0):
    """the host side of a case: sequences, cloud rows from the cloud's restatement, and what does not depend on the fill"""
    rng = np.random.default_rng([21, seed])
    seqs = []
    for b in range(B):
        pose = np.tile(np.eye(4, dtype=F).reshape(16), (3, 1))
        for k in range(3):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            pose[k].reshape(4, 4)[:3, :3] = q
            pose[k].reshape(4, 4)[:3, 3] = rng.uniform(-3, 3, 3)
        seqs.append(dict(depth=cases.random_depth(rng, (FRAMES, ROWS, COLS), depth_type), n_images=N_IMAGES[b], pose=pose,
                         frame_index=np.array([2, 0], np.int32)))
    rows = None
    if with_rows:
        scale = 1e-3 if depth_type == "u16" else 1.0
        stride = max(cloud_ref.depth_cloud(s, cloud_ref.params(K, scale=scale), FRAMES * ROWS * COLS)["n_out"] for s in seqs)
        rows = []
        for s in seqs:
            c = cloud_ref.depth_cloud(s, cloud_ref.params(K, scale=scale), stride)
            rows.append(dict(frame=c["frame"], pixel=c["pixel"], n=c["n_out"], base=None))
        assert rows[-1]["n"] == stride  # the full sequence's last row is the array's last
    return seqs, rows


def run_case(hip_ctx, arena, depth_type, radius, smooth, with_rows, shrink=None):
    """builds the arrays in the arena, runs, compares with the restatement -> the outputs.  shrink: the name of an array whose extent
    is understated by 16 bytes"""
    fill = arena.fill
    u16 = depth_type == "u16"
    np_dtype, t_dtype, es = (np.uint16, torch.uint16, 2) if u16 else (F, torch.float32, 4)
    scale = 1e-3 if u16 else 1.0
    seqs, rows = build(depth_type, with_rows)
    pitch = COLS + 2

    def put(name, host, dtype, align, extent=None):
        host = np.ascontiguousarray(host)
        full = host.nbytes if extent is None else extent
        t = arena.take(host.shape, dtype, align, name, extent=full - (16 if name == shrink else 0))
        t.copy_(torch.from_numpy(host))
        return t

    depth = filled((B, FRAMES, ROWS, pitch), np_dtype, fill)
    for b, s in enumerate(seqs):
        depth[b, :s["n_images"], :, :COLS] = s["depth"][:s["n_images"]]
    t = dict(depth=put("depth", depth, t_dtype, es, ((B * FRAMES * ROWS - 1) * pitch + COLS) * es),
             n_images=put("n_images", np.array(N_IMAGES, np.int32), torch.int32, 4))
    out = dict(normal=put("normal", filled((B, FRAMES, ROWS, COLS, 4), F, fill), torch.float32, 16),
               n_normal=put("n_normal", filled((B, FRAMES), np.int32, fill), torch.int32, 4),
               status=put("status", filled((B,), np.int32, fill), torch.int32, 4))
    d = _lib_normals.DepthNormalsBatch()
    d.batch, d.frames, d.rows, d.cols, d.pitch = B, FRAMES, ROWS, COLS, pitch * es
    d.depth, d.n_images = t["depth"].data_ptr(), t["n_images"].data_ptr()
    if with_rows:
        stride = len(rows[0]["frame"])
        frame, pixel = filled((B, stride), np.int32, fill), filled((B, stride), np.int32, fill)
        for b, r in enumerate(rows):
            frame[b, :r["n"]], pixel[b, :r["n"]] = r["frame"][:r["n"]], r["pixel"][:r["n"]]
            r["frame"], r["pixel"] = frame[b], pixel[b]
        t.update(pose=put("pose", np.stack([s["pose"] for s in seqs]), torch.float32, 4),
                 frame_index=put("frame_index", np.stack([s["frame_index"] for s in seqs]), torch.int32, 4),
                 row_frame=put("row_frame", frame, torch.int32, 4), row_pixel=put("row_pixel", pixel, torch.int32, 4),
                 row_n=put("row_n", np.array([r["n"] for r in rows], np.int32), torch.int32, 4))
        out.update(row_normal=put("row_normal", filled((B, stride, 4), F, fill), torch.float32, 16),
                   n_bad_rows=put("n_bad_rows", filled((B,), np.int32, fill), torch.int32, 4))
        d.pose_stride, d.row_stride = 3, stride
        for name in ("pose", "frame_index", "row_frame", "row_pixel", "row_n"):
            setattr(d, name, t[name].data_ptr())
    for name, tensor in out.items():
        setattr(d, name, tensor.data_ptr())
    p = ops.depth_normals_params(K, radius, smooth, depth_type=depth_type, scale=scale)
    assert _lib_normals.load().prs_depth_normals_batch_run(hip_ctx._h, C.byref(p), C.byref(d)) == 0
    hip_ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    rp = ref.params(K, radius, smooth, scale=scale)
    for b, s in enumerate(seqs):
        before = dict(normal=filled((FRAMES, ROWS, COLS, 4), F, fill), n_normal=filled((FRAMES,), np.int32, fill))
        if with_rows:
            before["row_normal"] = filled((stride, 4), F, fill)
        want = ref.depth_normals(s, rp, before, rows[b] if with_rows else None)
        assert int(got["status"][b]) == want["status"] == 0
        for k in ("normal", "n_normal", "row_normal"):
            if k in want:
                assert got[k][b].tobytes() == want[k].tobytes(), (b, k)
        if with_rows:
            assert int(got["n_bad_rows"][b]) == want["n_bad_rows"] == 0
            assert (want["row_normal"][:rows[b]["n"], 3] > 0).sum() > 50
        assert want["n_normal"][:s["n_images"]].min() > 50  # radius 8 finds few in an image with a step every 7 columns
    return got


@pytest.mark.parametrize("with_rows", [False, True], ids=["images", "rows"])
@pytest.mark.parametrize("setting", [(2, 1), (8, 3), (1, 0)], ids=lambda s: "r%d_s%d" % s)
@pytest.mark.parametrize("depth_type", ["u16", "f32"])
def test_depth_normals(hip_ctx, depth_type, setting, with_rows):
    guarded.both_fills(lambda arena: run_case(hip_ctx, arena, depth_type, setting[0], setting[1], with_rows))


@pytest.mark.parametrize("name", ["normal", "row_normal"])
def test_an_understated_extent_is_reported(hip_ctx, name):
    """the harness believes the array to end 16 bytes early: the last pixel's, or the last row's, store lands in the band"""
    arena = guarded.Arena(0xFF)  # whatever the call stores there, zeros included, is not the fill
    run_case(hip_ctx, arena, "f32", 2, 1, True, shrink=name)
    with pytest.raises(guarded.Violation) as report:
        arena.check()
    assert name in str(report.value) and "after" in str(report.value)
