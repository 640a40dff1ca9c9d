"""Front-end entry points inside guard bands (tests/guarded.py) at the buffer sizes and alignments include/proslam_hip.h documents:
prs_stereo_match_batch, prs_triangulate_dev, prs_bruteforce_match_batch and prs_scene_clip_batch.  One case each; the last frame,
pair or scene is the full one, so its counts equal the strides and its last row adjoins a band.  Each case runs with fill 0x00 and
with fill 0xFF, equals the oracle as the stage's own test asserts it, gives the same bytes in both runs and leaves every band
clean.  The two feature extractors and prs_align_batch_run: tests/test_guard_tracking_gpu.py.  What stays invisible to these cases: a
read past an array's end whose value reaches no result, and memory the library owns (the context's scratch arenas), which
cannot be placed."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded
import helpers as hp
import test_scene_clip_edges_gpu as clip
import test_stereo_match_gpu as stereo
from helpers import oracle_tri_params
from srrg2_proslam_amd import _lib, configs, ops, synthetic as syn

pytestmark = pytest.mark.gpu
F = np.float32
cc = clip.cc


def numpy_of(obj, names):
    return {k: getattr(obj, k).cpu().numpy() for k in names if getattr(obj, k) is not None}


def test_stereo_match_batch_counts_at_the_strides(oracle, hip_ctx):
    """the stage's own batched case: twelve frames at stride 2000, the last one (and two others) with 2000 keypoints on either side,
    the fused adaptor and triangulator outputs on"""
    names = ("matches", "n_matches", "status", "fixed_uvuv", "fixed_desc", "n_fixed", "fixed_xyz")

    def case(arena):
        frames = []

        def slack(f):  # upload writes the first n rows of the inputs; rows from the count to the stride are not read
            for t in (f.left_kp, f.right_kp, f.left_desc, f.right_desc, f.matches, f.fixed_uvuv, f.fixed_desc, f.fixed_xyz):
                arena.paint(t)
            frames.append(f)

        with guarded.hooked(arena, ops.StereoFrames, after=slack):
            stereo.test_batched_device_api_with_fused_adaptor_and_triangulator(oracle, hip_ctx, 0)
        f, = frames
        assert f.n_left.tolist()[-1] == f.n_right.tolist()[-1] == f.stride and all(arena.owns(getattr(f, k)) for k in names)
        return numpy_of(f, names)

    guarded.both_fills(case, nbytes=64 << 20)


def test_triangulate_dev(oracle, hip_ctx):
    """4097 measurements in arrays of exactly 4097 rows; a pointer that is only 4-byte aligned is refused, nothing launched"""
    cfg, n = configs.get("kitti"), 4097
    rng = np.random.default_rng(21)
    u, v, ur = syn.project_left_right(cfg["camera"], syn.sample_landmarks(rng, cfg["camera"], cfg["depth"], n))
    uvuv = np.stack([u, v, ur, v + rng.integers(-1, 2, n)], axis=1).astype(F)
    uvuv[::7, 2] = uvuv[::7, 0]  # zero disparity
    want, valid = oracle.triangulate(uvuv, oracle_tri_params(oracle, cfg))
    tp = ops.triangulator_params(cfg)
    run = _lib.load().prs_triangulate_dev

    def case(arena):
        d_in, d_out = arena.take((n, 4), torch.float32, 16, "uvuv"), arena.take((n, 4), torch.float32, 16, "xyz4")
        d_in.copy_(torch.from_numpy(uvuv))
        assert run(hip_ctx._h, C.byref(tp), d_in.data_ptr(), n, d_out.data_ptr()) == 0
        hip_ctx.synchronize()
        got = d_out.cpu().numpy()
        assert np.array_equal(got[:, :3].view(np.uint32), want.view(np.uint32)) and np.array_equal(got[:, 3] != 0, valid.astype(bool))
        for shift_in, shift_out in ((4, 0), (0, 4)):
            assert run(hip_ctx._h, C.byref(tp), d_in.data_ptr() + shift_in, n - 1, d_out.data_ptr() + shift_out) == _lib.ERR_UNSUPPORTED
        hip_ctx.synchronize()
        assert d_out.cpu().numpy().tobytes() == got.tobytes()
        return dict(xyz4=got)

    guarded.both_fills(case)


def test_bruteforce_match_batch_matches_at_their_stride(oracle, hip_ctx):
    """three cloud pairs at strides 257 x 257; the last is a cloud against itself: 257 matches, the stride of the output"""
    rng = np.random.default_rng(31)
    n = 257
    proto = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pairs = [(proto[:17].copy(), syn.flip_bits(rng, proto[:40], 0.02)), (syn.flip_bits(rng, proto[:100], 0.02), proto[50:150].copy()), (proto, proto)]
    want = [oracle.bruteforce_match(df, dm, 50.0, 0.9) for df, dm in pairs]
    names = ("matches", "n_matches", "status")

    def case(arena):
        made = []

        def slack(c):
            for t in (c.fixed_desc, c.moving_desc, c.matches):
                arena.paint(t)
            made.append(c)

        with guarded.hooked(arena, ops.BruteforceClouds, after=slack):
            clouds = ops.BruteforceClouds(0, len(pairs), n, n, candidate_capacity=n * n)
        for b, (df, dm) in enumerate(pairs):
            clouds.upload(b, df, dm)
        ops.bruteforce_match_batch(hip_ctx, ops.bruteforce_params(50.0, 0.9), clouds)
        hip_ctx.synchronize()
        for b, (ref, flags) in enumerate(want):
            assert hp.corr_equal(ref, clouds.matches_of(b)) and int(clouds.status[b].item()) == flags, b
        assert clouds.n_matches.tolist()[-1] == clouds.out_stride == n and made == [clouds]
        return numpy_of(clouds, names)

    guarded.both_fills(case)


@pytest.mark.parametrize("stride", [1025, 2049], ids=["walk", "count_and_scatter"])
def test_scene_clip_batch_scene_at_its_stride(hip_ctx, monkeypatch, stride):
    """three scenes in arrays of exactly three; the last has n_scene == stride.  Two tiles take the walk, three count + scatter"""
    assert clip.shape_of(3, stride) == ("walk" if stride == 1025 else "count+scatter")

    def batch_for(fill):
        rng = np.random.default_rng(41 + stride)
        batch = cc.blank("guard-%d-%d" % (stride, fill), 3, stride, "tall", cc.I4)
        c = cc.edge_cloud("tall")
        k = min(stride, len(c["xyzw"]))
        cc.put_scene(batch, 0, "edges", c["xyzw"][:k], c["desc"][:k])
        cc.put_scene(batch, 1, "short", cc.random_cloud(rng, stride - 300, "tall"))
        cc.put_scene(batch, 2, "full", cc.random_cloud(rng, stride, "tall"), R=cc.general_pose(rng, 0.2))
        for b in range(3):  # rows from n_scene to the stride
            batch["xyzw"][b, batch["n_scene"][b]:] = guarded.host_fill(F, fill)
            batch["desc"][b, batch["n_scene"][b]:] = fill
        return batch

    def case(arena):
        monkeypatch.setattr(clip, "SENTINEL", arena.fill)
        monkeypatch.setattr(clip, "SENTINEL32", int.from_bytes(bytes([arena.fill] * 4), "little"))
        batch = batch_for(arena.fill)
        with guarded.hooked(arena, ops.ClipScenes):
            sc = ops.ClipScenes(0, 3, stride)
        clip.put(sc, batch)
        out = clip.launch(hip_ctx, sc, batch)
        clip.check(out, batch)
        assert int(out[3][2]) > 0 and batch["n_scene"][2] == stride
        return dict(zip(("xyzw", "desc", "idx", "count", "status"), out))

    guarded.both_fills(case)
