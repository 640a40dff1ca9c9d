"""GPU parity of the selective extractor (IntensityFeatureExtractorSelective_) through the C-ABI: the reference's own counts
on KITTI city_left[0] (srrg2_proslam/tests/test_feature_extractors.cpp:168-262), and keypoints (order included), intensities
and descriptors byte-equal to the CPU checker (tests/selective_ref.py) on batches of KITTI, ICL and random images with
0 .. 2000 projections under every flag combination; the documented status codes at the capacity edges; the C++ adapter."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ref_pins as rp
import selective_ref as sr
from srrg2_proslam_amd import ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRS_WARN_NO_MATCHES, PRS_ERR_CAPACITY, PRS_ERR_RANGE, PRS_ERR_UNSUPPORTED = 2, -2, -4, -5


def _same(got, ref):
    assert len(got[0]) == len(ref[0])
    assert np.array_equal(got[0], ref[0])  # keypoints, in order
    assert np.array_equal(got[1], ref[1])  # intensities
    assert np.array_equal(got[2], ref[2])  # descriptors


@pytest.mark.parametrize("descriptor", ["ORB-256", "BRIEF-256"])
def test_reference_counts_and_checker_parity(hip_ctx, descriptor):
    img = rp.kitti_image("left", 0)
    eig = sr.min_eigen(img)
    p = ops.selective_extractor_params("GFTT", descriptor, 100, 10, enable_seeding_when_tracking=False)
    seeded = ops.extract_features_selective(hip_ctx, p, img)
    assert len(seeded[0]) == 94
    _same(seeded, sr.extract(img, 100, 10, eig=eig))
    p = ops.selective_extractor_params("GFTT", descriptor, 1000, 10, enable_seeding_when_tracking=False)
    for radius, expected in ((100, 719), (50, 581), (10, 294), (5, 237)):
        got = ops.extract_features_selective(hip_ctx, p, img, projections=seeded[0], radius=radius)
        assert len(got[0]) == expected, radius
        _same(got, sr.extract(img, 1000, 10, projections=seeded[0], radius=radius, seeding_when_tracking=False, eig=eig))


def _run_batch(hip_ctx, params, images, projections, radius, stride=4096, masks=None):
    dev = torch.device("cuda", 0)
    B = len(images)
    P = max(1, max(len(q) for q in projections))
    proj = np.zeros((B, P, 2), np.float32)
    for b, q in enumerate(projections):
        proj[b, :len(q)] = q
    img = torch.from_numpy(np.stack(images)).to(dev).contiguous()
    kp = torch.zeros((B, stride, 2), dtype=torch.float32, device=dev)
    desc = torch.zeros((B, stride, 32), dtype=torch.uint8, device=dev)
    inten = torch.zeros((B, stride), dtype=torch.float32, device=dev)
    n = torch.full((B,), -7, dtype=torch.int32, device=dev)
    st = torch.full((B,), -7, dtype=torch.int32, device=dev)
    tp = torch.from_numpy(proj).to(dev)
    tn = torch.tensor([len(q) for q in projections], dtype=torch.int32, device=dev)
    tr = torch.tensor(radius, dtype=torch.int32, device=dev)
    tm = torch.from_numpy(np.stack(masks)).to(dev).contiguous() if masks is not None else None
    ops.extract_features_selective_batch(hip_ctx, params, img, kp, desc, n, st, inten, projections=tp, n_projections=tn, radius=tr, seeding_mask=tm)
    hip_ctx.synchronize()
    return kp.cpu().numpy(), desc.cpu().numpy(), inten.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy()


def _projections(rng, rows, cols, count):
    uv = np.stack([rng.uniform(0, cols - 0.5, count), rng.uniform(0, rows - 0.5, count)], 1).astype(np.float32)
    uv[: count // 4] = np.floor(uv[: count // 4]) + np.float32(0.5)  # half-pixel positions: std::round away from zero
    return uv


def _image_sets():
    rng = np.random.default_rng(5)
    kitti = [rp.kitti_image("left", i) for i in range(3)] + [rp.kitti_image("right", 1)]
    icl = [rp.icl_gray(k) for k in (0, 1, 50)] + [rp.icl_gray(0)[::-1].copy()]
    noise = [rng.integers(0, 256, (120, 200)).astype(np.uint8) for _ in range(3)]
    noise.append(np.repeat(np.repeat(rng.integers(0, 256, (30, 50)), 4, 0), 4, 1).astype(np.uint8))  # blocky: many ties
    return {"kitti": kitti, "icl": icl, "random": noise}


@pytest.mark.parametrize("left,right", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("seeding", [False, True])
@pytest.mark.parametrize("name", ["kitti", "icl", "random"])
def test_mixed_batches_equal_the_checker(hip_ctx, name, left, right, seeding):
    images = _image_sets()[name]
    rows, cols = images[0].shape
    rng = np.random.default_rng(100 + 8 * int(left) + 4 * int(right) + 2 * int(seeding))
    counts = [0, 1, 300, 2000]
    projections = [_projections(rng, rows, cols, c) for c in counts]
    radius = [0, 5, 50, 0]
    target, width = (600, 10) if name != "random" else (300, 4)
    p = ops.selective_extractor_params("GFTT", "ORB-256", target, width, left, right, seeding, max_candidates=16384)
    kp, desc, inten, n, st = _run_batch(hip_ctx, p, images, projections, radius)
    for b, img in enumerate(images):
        ref = sr.extract(img, target, width, projections=projections[b], radius=radius[b], full_left=left, full_right=right,
                         seeding_when_tracking=seeding)
        assert st[b] == (0 if len(ref[0]) else PRS_WARN_NO_MATCHES), (b, st[b])
        k = int(n[b])
        _same((kp[b, :k], inten[b, :k], desc[b, :k]), ref)


def test_external_seeding_mask_in_a_batch(hip_ctx):
    images = _image_sets()["kitti"]
    rows, cols = images[0].shape
    rng = np.random.default_rng(9)
    masks = [(rng.uniform(size=(rows, cols)) < f).astype(np.uint8) for f in (0.0, 0.3, 1.0, 0.5)]
    masks[1][:, : cols // 2] = 0
    projections = [np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), _projections(rng, rows, cols, 50)]
    p = ops.selective_extractor_params("GFTT", "ORB-256", 500, 10)
    kp, desc, inten, n, st = _run_batch(hip_ctx, p, images, projections, [0, 0, 0, 20], masks=masks)
    assert st[0] == PRS_WARN_NO_MATCHES and n[0] == 0  # an all-zero mask detects nothing
    for b, img in enumerate(images):
        ref = sr.extract(img, 500, 10, projections=projections[b], radius=[0, 0, 0, 20][b], external_mask=masks[b])
        k = int(n[b])
        _same((kp[b, :k], inten[b, :k], desc[b, :k]), ref)


def test_capacity_edges(hip_ctx):
    img = rp.kitti_image("left", 0)
    ref = sr.extract(img, 1000, 10)
    # features: exactly stride fits, one fewer fails the image (and only that image)
    flat = np.zeros_like(img)
    p = ops.selective_extractor_params("GFTT", "ORB-256", 1000, 10)
    k = len(ref[0])
    for stride, status in ((k, 0), (k - 1, PRS_ERR_CAPACITY)):
        kp, desc, inten, n, st = _run_batch(hip_ctx, p, [img, flat], [np.zeros((0, 2), np.float32)] * 2, [0, 0], stride=stride)
        assert st[0] == status and st[1] == PRS_WARN_NO_MATCHES and n[1] == 0  # a flat image has no corner at all
        assert n[0] == (k if status == 0 else 0)
    # candidates: exactly max_candidates fit, one more fails
    nc = len(sr.candidates(img, None)[0])
    for cap, status in ((nc, 0), (nc - 1, PRS_ERR_CAPACITY)):
        p = ops.selective_extractor_params("GFTT", "ORB-256", 1000, 10, max_candidates=cap)
        kp, desc, inten, n, st = _run_batch(hip_ctx, p, [img], [np.zeros((0, 2), np.float32)], [0])
        assert st[0] == status
    with pytest.raises(ops.ProslamHipError) as e:
        ops.extract_features_selective(hip_ctx, ops.selective_extractor_params("GFTT", "ORB-256", 1000, 10), img, capacity=k - 1)
    assert e.value.status == PRS_ERR_CAPACITY


def test_unsupported_and_out_of_range(hip_ctx):
    img = rp.kitti_image("left", 0)
    with pytest.raises(ops.ProslamHipError) as e:
        ops.extract_features_selective(hip_ctx, ops.selective_extractor_params("FAST"), img)
    assert e.value.status == PRS_ERR_UNSUPPORTED
    with pytest.raises(ops.ProslamHipError) as e:
        ops.extract_features_selective(hip_ctx, ops.selective_extractor_params("GFTT"), img, projections=[(float(img.shape[1]), 10.0)])
    assert e.value.status == PRS_ERR_RANGE
    flat = np.zeros_like(img)
    assert len(ops.extract_features_selective(hip_ctx, ops.selective_extractor_params("GFTT"), flat)[0]) == 0  # PRS_WARN_NO_MATCHES


def test_cpp_selective_adapter(tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "test_selective_plugin")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    img = rp.kitti_image("left", 0)
    raw = tmp_path / "city_left_0.raw"
    raw.write_bytes(np.ascontiguousarray(img).tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, str(raw), str(img.shape[0]), str(img.shape[1])], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert out.count("[  OK  ]") == 5 and "FAILED" not in out and "0 failure(s)" in out, out
