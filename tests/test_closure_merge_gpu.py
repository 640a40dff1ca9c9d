"""The closure merger on the device (csrc/closure_merge.hip) against the numpy restatement of its rule (tests/closure_merge_ref.py):
every array of the scene over its whole capacity, the count and the result must be byte-identical.  Cases: tests/closure_merge_cases.py
(tests/test_closure_merge_ref.py checks on the CPU that each one exercises what its name says)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import closure_merge_cases as cc
import closure_merge_ref as cr
import point_align_ref as par
from srrg2_proslam_amd import _lib, configs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def params_of(P):
    p = _lib.ClosureMergerParams()
    for k, v in P.items():
        setattr(p, k, v)
    return p


def run_batch(ctx, ops, cases, uploads=None, with_gate=False, accepted=None, stride=None):
    """cases of one capacity and one set of parameters in ONE launch -> [(scene after, result)]"""
    cap = cases[0]["scene"]["coords"].shape[0]
    assert all(c["scene"]["coords"].shape[0] == cap for c in cases)
    ms = stride or max(max(len(c["measurement"]) for c in cases), 1)
    cs = stride or max(max(len(c["corr"]) for c in cases), 1)
    mb = ops.ClosureMergeBatch(0, len(cases), cap, ms, cs, with_stats="state" in cases[0]["scene"], with_gate=with_gate)
    mb.corr_from_aligner = cases[0].get("corr_from_aligner", 0)
    mb.transform_is_scene_in_measurement = cases[0].get("transform_is_scene_in_measurement", 0)
    for b, c in enumerate(cases):
        mb.upload(b, c["scene"], c["measurement"], c["measurement_desc"], c["corr"], c["transform"], c.get("scene_in_world"),
                  accepted=None if accepted is None else accepted[b], **((uploads or [{}] * len(cases))[b]))
    ops.closure_merge_batch(ctx, params_of(cases[0]["P"]), mb)
    ctx.synchronize()
    return [(mb.scene_of(b), mb.result_of(b)) for b in range(len(cases))]


def assert_same(got, res, want, want_res, what):
    assert res == want_res, (what, res, want_res)
    assert got["n_points"] == want["n_points"], what
    assert set(got) == set(want), what
    for k in want:
        if k != "n_points":
            if got[k].tobytes() != want[k].tobytes():
                bad = np.nonzero((got[k].reshape(len(got[k]), -1) != want[k].reshape(len(want[k]), -1)).any(axis=1))[0]
                raise AssertionError("%s: %s differs in rows %s" % (what, k, bad[:10]))


@pytest.mark.parametrize("kind", [cr.UVD, cr.XYZ])
@pytest.mark.parametrize("frame,distance2,target,binning,wanted", cc.ICL_CASES)
def test_icl_frames(env, frame, distance2, target, binning, wanted, kind):
    ctx, ops, B = env
    c = cc.icl_case(B, frame, distance2, target, binning, kind)
    S, r, _ = cc.want(c)
    (got, res), = run_batch(ctx, ops, [c])
    assert_same(got, res, S, r, "icl")
    assert (got["n_points"], res[0], res[1]) == wanted  # the reference's pins and the cap (tests/test_mergers.cpp:195, :232)


@pytest.mark.parametrize("name", sorted(cc.EDGES))
def test_synthetic_edges(env, name):
    ctx, ops, _ = env
    c = cc.edge(name)
    S, r, _ = cc.want(c)
    (got, res), = run_batch(ctx, ops, [c])
    assert_same(got, res, S, r, name)


def test_several_pairs_in_one_launch(env):
    """the n_corr family shares its shapes: six workgroups, each pair as it is alone"""
    ctx, ops, _ = env
    cases = [cc.edge("n_corr_%d" % n) for n in (257, 0, 65, 1, 64, 63)]
    for c, (got, res) in zip(cases, run_batch(ctx, ops, cases)):
        S, r, _ = cc.want(c)
        assert_same(got, res, S, r, c["name"])


def test_errors_leave_what_the_header_promises(env):
    ctx, ops, _ = env
    items = cc.error_batch()
    out = run_batch(ctx, ops, [c for c, _, _ in items], uploads=[kw for _, kw, _ in items], stride=128)
    assert [res[2] for _, res in out] == [cr.ERR_RANGE, cr.ERR_CAPACITY, cr.ERR_DUPLICATE, cr.ERR_SCENE_FULL, cr.OK]
    for (c, kw, code), (got, res) in zip(items, out):
        S, r, _ = cc.want(c, **kw)
        assert_same(got, res, S, r, "error %d" % code)
        if code in (cr.ERR_RANGE, cr.ERR_CAPACITY, cr.ERR_DUPLICATE):
            assert cr.scenes_equal(got, c["scene"]) and res[:2] == (0, 0)
        elif code == cr.ERR_SCENE_FULL:
            assert res[0] > 0 and res[1] == 0 and got["n_points"] == c["scene"]["n_points"]


def test_negative_counts(env):
    ctx, ops, _ = env
    base = dict(n_scene=100, n_meas=120, n_corr=60, target=1000, capacity=256)
    cases = [cc.synthetic(seed=60 + i, **base) for i in range(4)]
    cases[3]["scene"] = dict(cases[3]["scene"], n_points=257)
    uploads = [dict(n_measured=-1), dict(n_corr=-1), dict(n_corr=129), {}]
    out = run_batch(ctx, ops, cases, uploads=uploads, stride=128)
    assert [res for _, res in out] == [(0, 0, cr.ERR_RANGE), (0, 0, cr.ERR_RANGE), (0, 0, cr.ERR_CAPACITY), (0, 0, cr.ERR_RANGE)]
    for c, (got, _) in zip(cases, out):
        assert cr.scenes_equal(got, c["scene"])


def test_gate(env):
    ctx, ops, _ = env
    cases = [cc.edge("n_corr_%d" % n) for n in (63, 64, 65, 257)]
    accepted = [1, 0, 7, 0]
    for c, a, (got, res) in zip(cases, accepted, run_batch(ctx, ops, cases, with_gate=True, accepted=accepted)):
        if a:
            S, r, _ = cc.want(c)
            assert_same(got, res, S, r, c["name"])
            assert res[0] > 0
        else:
            assert res == (0, 0, cr.OK) and cr.scenes_equal(got, c["scene"])


def test_call_level_refusals(env):
    ctx, ops, _ = env
    c = cc.edge("n_measured_1")
    P = params_of(c["P"])
    for build, code in ((lambda: ops.ClosureMergeBatch(0, 1, 64, 16385, 8), _lib.ERR_UNSUPPORTED),   # measurement_stride above 16384
                        (lambda: ops.ClosureMergeBatch(0, 1, 1 << 19, 64, 8, with_stats=False), _lib.ERR_UNSUPPORTED)):  # scene bitmap of 64 KiB
        with pytest.raises(_lib.ProslamHipError) as e:
            ops.closure_merge_batch(ctx, P, build())
        assert e.value.status == code
    mb = ops.ClosureMergeBatch(0, 1, 64, 64, 8)
    mb.scene_in_world = None
    with pytest.raises(_lib.ProslamHipError) as e:
        ops.closure_merge_batch(ctx, P, mb)
    assert e.value.status == _lib.ERR_NULL
    bad = params_of(dict(c["P"], number_of_row_bins=0))
    with pytest.raises(_lib.ProslamHipError) as e:
        ops.closure_merge_batch(ctx, bad, ops.ClosureMergeBatch(0, 1, 64, 64, 8))
    assert e.value.status == _lib.ERR_UNSUPPORTED
    # the tracking mergers' entry keeps refusing what it does not serve
    mp = _lib.MergerParams()
    mp.variant = 3
    with pytest.raises(_lib.ProslamHipError):
        ops.merge_batch(ctx, mp, ops.MapBatch(0, 1, 64, 0, 4, 64, 64))


def test_graph_capture(env):
    import torch
    ctx, ops, _ = env
    c = cc.edge("transform")
    S, r, _ = cc.want(c)
    cap = c["scene"]["coords"].shape[0]
    mb = ops.ClosureMergeBatch(0, 1, cap, len(c["measurement"]), len(c["corr"]))
    up = lambda: mb.upload(0, c["scene"], c["measurement"], c["measurement_desc"], c["corr"], c["transform"], c["scene_in_world"])  # noqa: E731
    up()
    P = params_of(c["P"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        ops.closure_merge_batch(ctx, P, mb)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ops.closure_merge_batch(ctx, P, mb)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    up()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_same(mb.scene_of(0), mb.result_of(0), S, r, "replay")


def test_chain_after_the_loop_closure_batch(env):
    """the KITTI closures of test_closures_from_the_detector: city 00 (the candidate map) against city 00 again and city 01 (accepted)
    and highway 274 (rejected).  Matcher, aligner and merger are enqueued back to back; nothing is read before the end."""
    import torch
    ctx, ops, B = env
    sc = {s["name"]: s for s in par.scenarios(B)}
    pairs = [sc["kitti_00_00"], sc["kitti_00_01"], [u for u in par.unrelated(B) if u["name"] == "city00_highway274"][0]]
    k = configs.get("kitti")
    fs, cap = max(len(p["fixed"]) for p in pairs), 145 + 160
    lc = ops.LoopClosureBatch(0, 3, fs, cap)
    for b, p in enumerate(pairs):
        lc.upload(b, p["fixed"], p["fixed_desc"], p["moving"], p["moving_desc"])
    P = ops.closure_merger_params(k["closure_merger"], k["camera"], "xyz")
    mb = ops.ClosureMergeBatch.from_closures(lc)
    assert mb.coords.data_ptr() == lc.pairs.moving.data_ptr() and mb.corr.data_ptr() == lc.clouds.matches.data_ptr()
    before = [mb.scene_of(b) for b in range(3)]
    torch.cuda.synchronize()
    lc.run(ctx, ops.bruteforce_params(k["loop"]["maximum_descriptor_distance"], 0.9), ops.point_align_params(k["loop"]))
    ops.closure_merge_batch(ctx, P, mb)
    ctx.synchronize()
    assert [lc.pairs.result_of(b)["accepted"] for b in range(3)] == [1, 1, 0]
    Pd = {f: getattr(P, f) for f, _ in _lib.ClosureMergerParams._fields_}
    Pd.update({f: np.float32(Pd[f]) for f in ("fx", "fy", "cx", "cy", "maximum_distance_geometry_squared", "maximum_response")})
    for b, p in enumerate(pairs):
        got, res = mb.scene_of(b), mb.result_of(b)
        corr = lc.clouds.matches_of(b).astype(cr.CORR_DTYPE)
        z = np.zeros((fs, 4), np.float32)
        z[: len(p["fixed"]), :3] = p["fixed"]
        S, r = cr.closure_merge(Pd, before[b], z, lc.clouds.fixed_desc[b].cpu().numpy(), corr, lc.pairs.X_of(b),
                                transform_is_scene_in_measurement=1, corr_from_aligner=1, n_measured=len(p["fixed"]),
                                gate_accepted=lc.pairs.result_of(b)["accepted"])
        assert_same(got, res, S, r, p["name"])
    assert cr.scenes_equal(mb.scene_of(2), before[2]) and mb.result_of(2) == (0, 0, cr.OK)
    r0, r1 = mb.result_of(0), mb.result_of(1)
    assert r0 == (145, 0, cr.OK)  # the same frame again: every landmark merges, nothing to add
    print("city 01 into city 00: %d matches, %d merged, %d added" % (len(lc.clouds.matches_of(1)), r1[0], r1[1]))
    assert r1[0] > 0 and r1[1] == len(pairs[1]["fixed"]) - r1[0] and mb.scene_of(1)["n_points"] == 145 + r1[1]


def test_host_entry_equals_the_batch_entry(env):
    ctx, ops, _ = env
    for name in ("transform_inverse", "no_stats", "xyz_unbinned", "n_corr_0"):
        c = cc.edge(name)
        S, r, _ = cc.want(c)
        got, res = ops.closure_merge(ctx, params_of(c["P"]), c["scene"], c["measurement"], c["measurement_desc"], c["corr"], c["transform"],
                                     c.get("scene_in_world"), c.get("transform_is_scene_in_measurement", 0), c.get("corr_from_aligner", 0))
        assert_same(got, res, S, r, name)
    c, kw, code = cc.error_batch()[2]
    got, res = ops.closure_merge(ctx, params_of(c["P"]), c["scene"], c["measurement"], c["measurement_desc"], c["corr"], c["transform"],
                                 c["scene_in_world"], check=False)
    assert res == (0, 0, cr.ERR_DUPLICATE) and cr.scenes_equal(got, c["scene"])


def test_map_handle_equals_the_batch_entry(env):
    ctx, ops, B = env
    c = cc.icl_case(B, "01", 0.01, 250, 1)
    n = c["scene"]["n_points"]
    scene = cr.copy_scene(c["scene"])  # what set_scene makes of the cloud: state = coordinates, the rest zero
    S, r = cr.closure_merge(c["P"], scene, c["measurement"], c["measurement_desc"], c["corr"], c["transform"], scene_in_world=np.eye(4))
    m = ops.MapHandle(ctx, 512, max_measured=512)
    m.set_scene(scene["coords"][:n, :3], scene["desc"][:n])
    res = m.merge_closure(params_of(c["P"]), c["transform"], c["measurement"], c["measurement_desc"], c["corr"])
    assert res == r == (215, 35, cr.OK) and m.size()[0] == S["n_points"] == 356
    got = m.scene()
    k = S["n_points"]
    assert np.array_equal(got["coords"], S["coords"][:k, :3]) and np.array_equal(got["state"], S["state"][:k, :3])
    assert np.array_equal(got["desc"], S["desc"][:k]) and np.array_equal(got["n_opt"], S["n_opt"][:k]) and np.array_equal(got["inlier"], S["inlier"][:k])
    # a second closure into the grown map, with the aligner's conventions; then a refused one leaves the handle's count alone
    X = cc.rigid(9, 0.01, 0.02)
    corr = np.zeros(len(c["corr"]), cr.CORR_DTYPE)
    corr["fixed_idx"], corr["moving_idx"], corr["response"] = c["corr"]["moving_idx"], c["corr"]["fixed_idx"], c["corr"]["response"]
    S2, r2 = cr.closure_merge(c["P"], S, c["measurement"], c["measurement_desc"], corr, X, scene_in_world=np.eye(4),
                              transform_is_scene_in_measurement=1, corr_from_aligner=1)
    res2 = m.merge_closure(params_of(c["P"]), X, c["measurement"], c["measurement_desc"], corr, transform_is_scene_in_measurement=1, corr_from_aligner=1)
    assert res2 == r2 and r2[0] > 0 and np.array_equal(m.scene()["coords"], S2["coords"][: S2["n_points"], :3])
    corr["moving_idx"][5] = corr["moving_idx"][4]
    assert m.merge_closure(params_of(c["P"]), X, c["measurement"], c["measurement_desc"], corr, corr_from_aligner=1, check=False)[2] == cr.ERR_DUPLICATE
    assert m.size()[0] == S2["n_points"]
    m.close()


def run_plugin(kind, c, rows, cols):
    exe = os.path.join(ROOT, "tests", "cpp", "test_closure_merge_plugin")
    assert os.path.exists(exe), "build() did not produce the adapter test program"
    tmp = tempfile.mkdtemp()
    f = {n: os.path.join(tmp, "closure_merge_%s.bin" % n) for n in ("scene", "scene_desc", "meas", "meas_desc", "corr", "T", "out", "out_desc")}
    n = c["scene"]["n_points"]
    c["scene"]["coords"][:n, :3].astype(np.float32).tofile(f["scene"])
    c["scene"]["desc"][:n].tofile(f["scene_desc"])
    np.ascontiguousarray(c["measurement"][:, :3]).tofile(f["meas"])
    np.ascontiguousarray(c["measurement_desc"]).tofile(f["meas_desc"])
    np.ascontiguousarray(c["corr"]).tofile(f["corr"])
    np.asarray(c["transform"], np.float32).tofile(f["T"])
    P = c["P"]
    out = subprocess.run([exe, kind, str(n), str(len(c["measurement"])), str(len(c["corr"])), str(rows), str(cols)] +
                         [repr(float(P[x])) for x in ("fx", "fy", "cx", "cy")] +
                         [str(P["target_number_of_merges"]), repr(float(P["maximum_distance_geometry_squared"]))] +
                         [f[x] for x in ("scene", "scene_desc", "meas", "meas_desc", "corr", "T", "out", "out_desc")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout, np.fromfile(f["out"], np.float32).reshape(-1, 3), np.fromfile(f["out_desc"], np.uint8).reshape(-1, 32)


def test_plugin_adapters(env):
    """the reference's two gtests through MergerCorrespondenceProjectiveDepth3DHIP (tests/test_mergers.cpp:174-246: the first leaves
    the canvas unset) and a 3D cloud through MergerCorrespondencePointIntensityDescriptor3fHIP"""
    _, _, B = env
    for kind, c, rows, cols, points in (("uvd", cc.icl_case(B, "00", 0.25, 1000, 1), 0, 0, 321), ("uvd", cc.icl_case(B, "01", 0.25, 1000, 1), 480, 640, 431),
                                        ("xyz", cc.synthetic(seed=70, n_scene=100, n_meas=300, n_corr=30, kind=cr.XYZ, target=60, n_behind=40,
                                                             n_off_canvas=40), cc.ROWS, cc.COLS, None)):
        plain = dict(c, scene={k: c["scene"][k] for k in ("coords", "desc", "n_points")}, scene_in_world=None)
        plain["scene"] = cr.copy_scene(plain["scene"])
        plain["scene"]["coords"][:, 3] = 0
        plain["scene"]["n_opt"] = np.zeros(len(plain["scene"]["coords"]), np.uint32)
        if rows == 0:
            plain["P"] = dict(c["P"], enable_binning=0)
        S, r, _ = cc.want(plain)
        text, xyz, desc = run_plugin(kind, plain, rows, cols)
        assert "points %d merged %d added %d" % (S["n_points"], r[0], r[1]) in text and "all checks passed" in text, text
        assert points is None or S["n_points"] == points
        assert np.array_equal(xyz, S["coords"][: S["n_points"], :3]) and np.array_equal(desc, S["desc"][: S["n_points"]])
