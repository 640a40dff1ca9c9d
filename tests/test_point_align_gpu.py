"""The loop aligner on the device (prs_point_align_batch / prs_point_align) equals the CPU checker (tests/point_align_ref.py) bit
for bit -- X, H, b, chi sums, counts, status, verdict, inlier mask -- and holds the pose bounds of the reference's loop-closing
gtests (test_loop_closing.cpp:19-284)."""
import numpy as np
import pytest

import point_align_ref as par
from oracle import binding as ob
from srrg2_proslam_amd import _lib, configs

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 1000, 8192]


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import ops
    from test_ref_pins import OracleBackend
    assert torch.cuda.is_available()
    ctx = ops.Context(0)
    yield ctx, ops, OracleBackend()
    ctx.close()


def assert_same(X, res, mask, Xr, rr, mr, what=""):
    assert np.array_equal(np.asarray(X, np.float32).reshape(4, 4).view(np.uint32), np.asarray(Xr, np.float32).view(np.uint32)), what
    assert np.array_equal(res["H"].view(np.uint32), rr["H"].view(np.uint32)), what
    assert np.array_equal(res["b"].view(np.uint32), rr["b"].view(np.uint32)), what
    for k in ("chi_inliers", "chi_total"):
        assert np.float32(res[k]).view(np.uint32) == np.float32(rr[k]).view(np.uint32), (what, k)
    for k in ("num_inliers", "num_outliers", "num_invalid", "num_correspondences", "status", "accepted", "iterations", "warnings"):
        assert res[k] == rr[k], (what, k, res[k], rr[k])
    if mr is not None and mask is not None:
        assert np.array_equal(mask, mr), what


def synthetic(rng, n, n_points=None, outliers=0.3):
    n_points = max(n, 1) if n_points is None else n_points
    moving = (rng.uniform(-20, 20, (n_points, 3)) + [0, 0, 30]).astype(np.float32)
    T = ob.tnq2t(np.array([0.3, -0.2, 0.5, 0.02, -0.03, 0.05], np.float32)).astype(np.float64)
    fixed = (moving @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.02, moving.shape)).astype(np.float32)
    idx = rng.integers(0, n_points, n)
    corr = np.stack([idx, idx], 1).astype(np.int32)
    bad = rng.random(n) < outliers
    corr[bad, 1] = rng.integers(0, n_points, bad.sum())
    return fixed, moving, corr


GUESS = ob.tnq2t(np.array([0.27, -0.17, 0.47, 0.018, -0.027, 0.047], np.float32))


def run_batch(ctx, ops, params, items, corr_stride, with_status=False):
    """items: (fixed, moving, corr, X0[, match_status]) -> per-pair (X, result, mask) from the device"""
    fs = max(max(len(i[0]) for i in items), 1)
    ms = max(max(len(i[1]) for i in items), 1)
    pb = ops.PointAlignBatch(0, len(items), fs, ms, corr_stride, with_status=with_status)
    for b, it in enumerate(items):
        pb.upload(b, it[0], it[1], it[2], it[3])
        if with_status:
            pb.match_status[b] = it[4]
    ops.point_align_batch(ctx, params, pb)
    ctx.synchronize()
    return [(pb.X_of(b), pb.result_of(b), pb.mask_of(b)) for b in range(len(items))]


def checker_params(p):
    return par.params(robustifier=p.robustifier, chi_threshold=p.chi_threshold, damping=p.damping, max_iterations=p.max_iterations,
                      min_num_inliers=p.min_num_inliers, min_num_correspondences=p.min_num_correspondences,
                      relocalize_min_inliers=p.relocalize_min_inliers, relocalize_min_inliers_ratio=p.relocalize_min_inliers_ratio,
                      relocalize_max_chi_inliers=p.relocalize_max_chi_inliers, linearize_only=p.linearize_only)


@pytest.mark.parametrize("form", ["clamp", "saturated"])
def test_reference_scenarios_match_then_register_on_the_device(env, form):
    ctx, ops, B = env
    cases = par.scenarios(B) + par.unrelated(B)
    for config in ("kitti", "icl"):
        group = [c for c in cases if c["config"] == config]
        loop = dict(configs.get(config)["loop"], robustifier=form)
        dist = sorted({c["max_distance"] for c in group})
        for d in dist:
            sub = [c for c in group if c["max_distance"] == d]
            fs, ms = max(len(c["fixed"]) for c in sub), max(len(c["moving"]) for c in sub)
            lc = ops.LoopClosureBatch(0, len(sub), fs, ms, candidate_capacity=fs * ms)  # every pair may pass at distance 75
            for b, c in enumerate(sub):
                lc.upload(b, c["fixed"], c["fixed_desc"], c["moving"], c["moving_desc"])
            P = ops.point_align_params(loop)
            lc.run(ctx, ops.bruteforce_params(d, 0.9), P)
            ctx.synchronize()
            for b, c in enumerate(sub):
                corr = lc.clouds.matches_of(b)
                assert int(lc.clouds.status[b].item()) >= 0, c["name"]
                ref_corr, _ = ob.bruteforce_match(c["fixed_desc"], c["moving_desc"], d, 0.9)
                assert np.array_equal(corr["fixed_idx"], ref_corr["fixed_idx"]) and np.array_equal(corr["moving_idx"], ref_corr["moving_idx"])
                Xr, rr, mr = par.align(checker_params(P), np.eye(4), c["fixed"], c["moving"], ref_corr)
                X, res, mask = lc.pairs.X_of(b), lc.pairs.result_of(b), lc.pairs.mask_of(b)
                assert_same(X, res, mask, Xr, rr, mr, c["name"])
                if "bounds" in c:
                    assert res["accepted"] == 1, c["name"]
                    if c["truth"] is None:
                        assert np.linalg.norm(par.pose_error(X, np.eye(4))) < 1e-5
                    else:
                        assert (np.abs(par.pose_error(X, c["truth"])) < np.asarray(c["bounds"])).all(), c["name"]
                else:
                    assert res["accepted"] == 0, c["name"]


def test_euroc_saturated_form(env):
    ctx, ops, _ = env
    rng = np.random.default_rng(11)
    items = [synthetic(rng, n) + (GUESS,) for n in (40, 150, 700)]
    P = ops.point_align_params(configs.get("euroc")["loop"], max_iterations=30)
    assert P.robustifier == _lib.ROBUSTIFIER_SATURATED
    got = run_batch(ctx, ops, P, items, 1024)
    for it, (X, res, mask) in zip(items, got):
        assert_same(X, res, mask, *par.align(checker_params(P), it[3], it[0], it[1], it[2]))


@pytest.mark.parametrize("parked", [1, 4, 6])
def test_every_instantiation_at_its_edges(env, parked):
    ctx, ops, _ = env
    rng = np.random.default_rng(parked)
    items = [synthetic(rng, n, n_points=max(n, 8)) + (GUESS,) for n in SIZES]
    P = ops.point_align_params(configs.get("icl")["loop"], parked_per_lane=parked, chi_threshold=0.5)
    got = run_batch(ctx, ops, P, items, 8192)
    for n, it, (X, res, mask) in zip(SIZES, items, got):
        assert_same(X, res, mask, *par.align(checker_params(P), it[3], it[0], it[1], it[2]), what=n)
    assert got[SIZES.index(0)][1]["warnings"] == _lib.WARN_NO_MATCHES
    assert got[SIZES.index(8192)][1]["status"] == 1


def test_default_instantiation_by_stride(env):
    ctx, ops, _ = env
    rng = np.random.default_rng(5)
    P = ops.point_align_params(configs.get("kitti")["loop"], min_num_correspondences=0)
    for stride in (64, 256, 8192):  # K = 1, 4, 6
        items = [synthetic(rng, n) + (GUESS,) for n in (3, min(stride, 100), stride)]
        for it, (X, res, mask) in zip(items, run_batch(ctx, ops, P, items, stride)):
            assert_same(X, res, mask, *par.align(checker_params(P), it[3], it[0], it[1], it[2]), what=stride)


def test_thresholds_at_their_boundaries(env):
    ctx, ops, B = env
    sc = par.scenarios(B)[1]  # KITTI 00 -> 01
    corr, _ = ob.bruteforce_match(sc["fixed_desc"], sc["moving_desc"], 25.0, 0.9)
    loop = configs.get("kitti")["loop"]
    f, m = sc["fixed"], sc["moving"]

    def run(c, **kw):
        P = ops.point_align_params(loop, **kw)
        X, res, mask, _ = ops.point_align(ctx, P, f, m, c, np.eye(4))
        assert_same(X, res, mask, *par.align(checker_params(P), np.eye(4), f, m, c))
        return res

    sub = corr[:30]
    assert [run(sub, min_num_correspondences=k)["iterations"] for k in (29, 30, 31)] == [100, 100, 0]
    base = run(corr)
    n_in, n = base["num_inliers"], base["num_correspondences"]
    assert base["accepted"] == 1
    assert [run(corr, min_num_inliers=k)["status"] for k in (n_in, n_in + 1)] == [1, 0]
    assert [run(corr, relocalize_min_inliers=k)["accepted"] for k in (n_in, n_in + 1)] == [1, 0]
    ratio = np.float32(n_in) / np.float32(n)
    assert [run(corr, relocalize_min_inliers_ratio=float(r))["accepted"] for r in (ratio, np.nextafter(ratio, np.float32(2)))] == [1, 0]
    chi = np.float32(base["chi_inliers"]) / np.float32(n_in)
    assert [run(corr, relocalize_max_chi_inliers=float(c))["accepted"] for c in (chi, np.nextafter(chi, np.float32(0)))] == [1, 0]


def test_bad_pairs_leave_their_neighbours_alone(env):
    ctx, ops, _ = env
    rng = np.random.default_rng(7)
    good = [synthetic(rng, n) + (GUESS, 0) for n in (50, 200, 90)]
    f, m, c = synthetic(rng, 80)
    f[3] = np.nan
    m[c[5, 1]] = np.inf
    nan_pair = (f, m, c, GUESS, 0)
    f2, m2, c2 = synthetic(rng, 60)
    c2 = c2.copy()
    c2[17, 0] = len(f2)
    bad_index = (f2, m2, c2, GUESS, 0)
    f3, m3, c3 = synthetic(rng, 60)
    bad_status = (f3, m3, c3, GUESS, -2)
    items = [good[0], nan_pair, good[1], bad_index, bad_status, good[2]]
    P = ops.point_align_params(configs.get("icl")["loop"], chi_threshold=0.5)
    got = run_batch(ctx, ops, P, items, 256, with_status=True)
    for i in (0, 1, 2, 5):
        it = items[i]
        assert_same(*got[i], *par.align(checker_params(P), it[3], it[0], it[1], it[2]), what=i)
    assert got[1][1]["num_invalid"] >= 2
    assert got[3][1]["warnings"] == _lib.ERR_RANGE and got[3][1]["iterations"] == 0
    assert got[4][1]["warnings"] == -2 and got[4][1]["iterations"] == 0
    for i in (3, 4):
        assert np.array_equal(got[i][0], np.asarray(GUESS, np.float32).reshape(4, 4))


def test_full_device_batch_and_its_permutation(env):
    import torch
    ctx, ops, _ = env
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(2024)
    sizes = rng.integers(0, 700, 2 * cus + 7)
    items = [synthetic(rng, int(n), n_points=max(int(n), 8)) + (GUESS,) for n in sizes]
    P = ops.point_align_params(configs.get("icl")["loop"], chi_threshold=0.5)
    got = run_batch(ctx, ops, P, items, 700)
    perm = rng.permutation(len(items))
    got_p = run_batch(ctx, ops, P, [items[i] for i in perm], 700)
    for j, i in enumerate(perm):
        assert_same(*got_p[j], *got[i], what=("perm", i))
    for i in range(0, len(items), 13):
        it = items[i]
        assert_same(*got[i], *par.align(checker_params(P), it[3], it[0], it[1], it[2]), what=i)


def test_host_entry_equals_batch_entry_and_linearize_only(env):
    ctx, ops, _ = env
    rng = np.random.default_rng(9)
    items = [synthetic(rng, n) + (GUESS,) for n in (7, 300)]
    for lin in (0, 1):
        P = ops.point_align_params(configs.get("kitti")["loop"], linearize_only=lin, min_num_correspondences=0)
        got = run_batch(ctx, ops, P, items, 512)
        for it, g in zip(items, got):
            X, res, mask, _ = ops.point_align(ctx, P, it[0], it[1], it[2], it[3])
            assert_same(X, res, mask, *g)
            assert_same(X, res, mask, *par.align(checker_params(P), it[3], it[0], it[1], it[2]))
            if lin:
                assert res["iterations"] == 1 and np.array_equal(X, np.asarray(GUESS, np.float32).reshape(4, 4))


def test_graph_capture_replays_the_launch(env):
    import torch
    ctx, ops, _ = env
    rng = np.random.default_rng(13)
    items = [synthetic(rng, n) + (GUESS,) for n in (33, 250, 600)]
    P = ops.point_align_params(configs.get("icl")["loop"], chi_threshold=0.5)
    pb = ops.PointAlignBatch(0, len(items), 600, 600, 600)
    for b, it in enumerate(items):
        pb.upload(b, it[0], it[1], it[2], it[3])
    X0 = pb.X.clone()
    ctx.use_torch_stream()
    ops.point_align_batch(ctx, P, pb)  # first call of the shape
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctx.use_torch_stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ops.point_align_batch(ctx, P, pb)
        pb.X.copy_(X0)
        pb.result.zero_()
        g.replay()
    torch.cuda.synchronize()
    ctx.use_torch_stream()
    for b, it in enumerate(items):
        assert_same(pb.X_of(b), pb.result_of(b), pb.mask_of(b), *par.align(checker_params(P), it[3], it[0], it[1], it[2]))


def test_cpp_adapter(env, tmp_path):
    import os
    import subprocess
    _, _, B = env
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "test_point_align_plugin")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    sc = par.scenarios(B)[1]  # KITTI 00 -> 01 with the adapter's kitti.conf defaults
    corr, _ = ob.bruteforce_match(sc["fixed_desc"], sc["moving_desc"], 25.0, 0.9)
    f, m = np.asarray(sc["fixed"], np.float32), np.asarray(sc["moving"], np.float32)
    c = np.stack([corr["fixed_idx"], corr["moving_idx"]], 1).astype(np.int32)
    (tmp_path / "in.bin").write_bytes(np.array([len(f), len(m), len(c)], np.int32).tobytes() + f.tobytes() + m.tobytes() + c.tobytes())
    env_ = dict(os.environ)
    env_["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env_.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=env_, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert out.count("[  OK  ]") == 3 and "0 failure(s)" in out, out
    raw = (tmp_path / "out.bin").read_bytes()
    X = np.frombuffer(raw[:64], np.float32).reshape(4, 4)
    rs = _lib.PointAlignResult.from_buffer_copy(raw[64:64 + C_RESULT])
    from srrg2_proslam_amd import ops
    mask = np.frombuffer(raw[64 + C_RESULT:], np.uint8)
    Xr, rr, mr = par.align(checker_params(ops.point_align_params(configs.get("kitti")["loop"])), np.eye(4), f, m, corr)
    assert_same(X, ops._result_dict(rs), mask, Xr, rr, mr)
    assert (np.abs(par.pose_error(X, sc["truth"])) < np.asarray(sc["bounds"])).all()


C_RESULT = __import__("ctypes").sizeof(_lib.PointAlignResult)


def test_zero_iterations_leave_the_pair_unlinearised(env):
    ctx, ops, _ = env
    rng = np.random.default_rng(17)
    f, m, c = synthetic(rng, 70)
    P = ops.point_align_params(configs.get("icl")["loop"], max_iterations=0)
    X, res, mask, _ = ops.point_align(ctx, P, f, m, c, GUESS)
    assert_same(X, res, mask, *par.align(checker_params(P), GUESS, f, m, c))
    assert res["iterations"] == 0 and res["status"] == 0 and not mask.any()
