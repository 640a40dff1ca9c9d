"""Every instantiation align_batch_launch (csrc/align.hip) dispatches to, against the CPU oracle and a float64 reference.

The dispatch picks a Gauss-Newton kernel (gn_kernel<SLOTS, DIM, KEEP_CLS, LDS_SLOTS, WAVES, PLAIN>) and a search kernel
(align_kernel<512, true, pattern, survivor slots>) from host-side facts no caller sees: batch size against two frames per CU
(the "lone" variants), max_fixed against 512 (SLOTS) and 1024 (split vs fused), the stereo factor and shipped forms ("fast"),
prior / with_sensor / inlier-only runs ("plain", motion-prior-only), the depth factor, and an LDS occupancy comparison (the survivor
slot width).  DISPATCH below names one row per instantiation with the knobs that select it; tests/test_align_dispatch_table.py
checks (without a GPU) that every instantiation in the library's variant table has a row and that the library's plan
(prs_align_plan) picks each row's kernels from the row's knobs.  Each row runs a batch of distinct frames and is
compared with the per-frame oracle bit for bit (correspondences incl. response bits, pose bits, status / warnings, finder state),
and every converged frame's final pose is checked to be a fixed point of a float64 Gauss-Newton step on its own correspondences.
Then the capacity edges (LDS-parked operand rows, max_fixed 512/513, 1024/1025, 2047/2048, a frame over its max_fixed), the pruned
scan's worst case (last database entry in the last scanned cell, correlated rows), the prune fallback hint in
prs_pcf_state.reserved and the bits of that word the library does not own."""
import numpy as np
import pytest

import ref_pins as rp
from helpers import aligner_params as oracle_aligner_params, corr_equal, make_align_case, pcf_params_from_cfg
from srrg2_proslam_amd import configs, ops, synthetic as syn

pytestmark = pytest.mark.gpu

MPRIOR_INFO = (3.0, 3.0, 3.0, 50.0, 50.0, 50.0)
SENSOR = syn.make_transform([0.12, -0.05, 0.3], [0.01, -0.02, 0.015]).astype(np.float32)
# A converged frame's final pose, linearised in float64 on its final correspondences, gives a Gauss-Newton step (translation m,
# quaternion imaginary part) below this: the CPU oracle's own results for these rows reach 4.3e-5 (inlier-only runs), <= 1e-6 otherwise
F64_STEP_TOL = 2e-4

# One row per instantiation of the dispatch.  gn / search: the kernels as a kernel trace prints them (the search kernel's last
# argument is the survivor slot width the LDS comparison gives at this max_fixed, SLOT_WIDTHS below; 4 for the KD-tree);
# no_lone: PRS_NO_LONE_GN=1; fused: PRS_FUSED_ALIGN=1.  mprior = motion prior (prior mean = the initial guess), sensor = with_sensor,
# akw / fkw = aligner / finder overrides (inlier-only runs, kept inlier classes, radius).
def GN(args):
    return "void prs::gn_kernel<%s>(prs::AlignArgs)" % args


def AK(args):
    return "void prs::align_kernel<%s>(prs::AlignArgs)" % args


# the survivor slot width of the lattice finders by max_fixed, for the rows' canvases and radii
SLOT_WIDTHS = {600: 4, 896: 4, 384: 8, 512: 8, 700: 8, 1000: 8, 1024: 8}
DISPATCH = [
    dict(id="lone4_plain", cfg="kitti", max_fixed=512, no_lone=0, gn=GN("4, 4, false, 4, 1, 1"), search=AK("512, true, 2, 8"), fkw=dict(search_type=2)),
    dict(id="lone4_mprior", cfg="kitti", max_fixed=512, no_lone=0, mprior=1, gn=GN("4, 4, false, 4, 1, 0"), search=AK("512, true, 1, 8"), fkw=dict(search_type=1)),
    dict(id="lone8_plain", cfg="kitti", max_fixed=600, no_lone=0, gn=GN("8, 4, false, 4, 1, 1"), search=AK("512, true, 2, 4"), fkw=dict(search_type=2, maximum_search_radius_pixels=100)),
    dict(id="lone8_sensor", cfg="kitti", max_fixed=896, no_lone=0, sensor=1, gn=GN("8, 4, false, 4, 1, 0"), search=AK("512, true, 1, 4"), fkw=dict(search_type=1, maximum_search_radius_pixels=100)),
    dict(id="tp4_plain", cfg="kitti", max_fixed=512, no_lone=1, gn=GN("4, 4, false, 4, 4, 1"), search=AK("512, true, 3, 8"), fkw=dict(search_type=3)),
    dict(id="tp4_mprior", cfg="kitti", max_fixed=448, no_lone=1, mprior=1, gn=GN("4, 4, false, 4, 4, 2"), search=AK("512, true, 0, 4"), fkw=dict(search_type=0)),
    dict(id="tp4_sensor", cfg="kitti", max_fixed=384, no_lone=1, sensor=1, gn=GN("4, 4, false, 4, 4, 0"), search=AK("512, true, 2, 8"), fkw=dict(search_type=2)),
    dict(id="depth4", cfg="tum", max_fixed=512, no_lone=0, gn=GN("4, 3, true, 4, 4, 0"), search=AK("512, true, 1, 8"), fkw=dict(search_type=1)),
    dict(id="generic4", cfg="euroc", max_fixed=512, no_lone=0, akw=dict(keep_only_inlier_correspondences=1), gn=GN("4, 0, true, 4, 4, 0"), search=AK("512, true, 3, 8"), fkw=dict(search_type=3)),
    dict(id="five_plain", cfg="kitti", max_fixed=896, no_lone=1, gn=GN("8, 4, false, 3, 5, 1"), search=AK("512, true, 3, 4"), fkw=dict(search_type=3, maximum_search_radius_pixels=100)),
    dict(id="five_mprior", cfg="kitti", max_fixed=1000, no_lone=1, mprior=1, gn=GN("8, 4, false, 3, 5, 2"), search=AK("512, true, 1, 8"), fkw=dict(search_type=1)),
    dict(id="five_inlier_runs", cfg="kitti", max_fixed=700, no_lone=1, akw=dict(enable_inlier_only_runs=1, inlier_only_iterations=5), gn=GN("8, 4, false, 3, 5, 0"), search=AK("512, true, 2, 8"), fkw=dict(search_type=2)),
    dict(id="depth8", cfg="tum", max_fixed=600, no_lone=0, gn=GN("8, 3, true, 4, 4, 0"), search=AK("512, true, 0, 4"), fkw=dict(search_type=0)),
    dict(id="generic8", cfg="euroc", max_fixed=1024, no_lone=0, akw=dict(keep_only_inlier_correspondences=1), gn=GN("8, 0, true, 4, 4, 0"), search=AK("512, true, 2, 8"), fkw=dict(search_type=2)),
    dict(id="fused_forced", cfg="kitti", max_fixed=800, no_lone=0, fused=1, gn=None, search=AK("256, false, -1, 4"), fkw=dict(search_type=2)),
    dict(id="fused_by_size", cfg="euroc", max_fixed=1100, no_lone=0, gn=None, search=AK("256, false, -1, 4"), fkw=dict(search_type=1)),
]
FRAMES_PER_ROW = 6


def row_kernels(row):
    """the kernels of a round as a plan lists them (search, Gauss-Newton); None for the ad-hoc rows of the edge tests"""
    return ([row["search"]] + ([row["gn"]] if row["gn"] else [])) if "search" in row else None


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _context(monkeypatch, no_lone=0, fused=0, no_prefilter=0):
    """a fresh context: the knobs are read when it is created"""
    for name, on in (("PRS_NO_LONE_GN", no_lone), ("PRS_FUSED_ALIGN", fused), ("PRS_NO_PREFILTER", no_prefilter)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)
    ctx = ops.Context(0)
    ctx.use_torch_stream()
    return ctx


def _cases(cfg_name, seed, n, max_fixed, n_kp=None, full=0):
    """n distinct frames whose fixed clouds fit max_fixed; the first `full` are cut to exactly max_fixed points"""
    out = []
    for b in range(n):
        k = n_kp or int(max_fixed * (1.6 if b < full else 1.1))
        cfg, fixed, dfix, mp, T, X0 = make_align_case(cfg_name, seed + b, k, k)
        cap = max_fixed if b < full else min(len(fixed), max_fixed)
        assert len(fixed) >= cap
        out.append(dict(fixed=fixed[:cap].copy(), dfix=dfix[:cap].copy(), xyz=mp["xyz"], dmov=mp["desc"], scale=None, X0=X0, n_opt=mp["n_opt"]))
    return configs.get(cfg_name), out


def _oracle_frame(oracle, cfg, c, fkw, akw, sensor=False, mprior=False, of=None, prior=None):
    if of is None:
        of = oracle.ProjectiveFinder(pcf_params_from_cfg(oracle, cfg, **fkw))
    of.set_fixed(c["fixed"], c["dfix"])
    of.set_moving(c["xyz"], c["dmov"])
    md = oracle.mean_disparity(c["fixed"]) if c["fixed"].shape[1] == 4 else 0.0
    oap = oracle_aligner_params(oracle, cfg, mean_disparity=md, **akw)
    if sensor:
        oap.with_sensor = 1
        for i, v in enumerate(SENSOR.reshape(16)):
            oap.sensor_in_robot[i] = float(v)
    if mprior:
        oap.enable_motion_prior = 1
        for i, v in enumerate(MPRIOR_INFO):
            oap.motion_prior_info[i] = v
    res, corr = oracle.align_frame(of, oap, c["fixed"], c["xyz"], c["scale"], c["X0"], prior=prior, prior_mean=c["X0"] if mprior else None)
    return of, res, corr


def _device_params(cfg, fkw, akw, sensor=False, mprior=False):
    ap = ops.aligner_params(cfg, stop_at_fixed_point=1, **akw)
    if sensor:
        ops.set_sensor_in_robot(ap, SENSOR)
    if mprior:
        ops.set_motion_prior(ap, MPRIOR_INFO)
    return ops.pcf_params(cfg, **fkw), ap


def _run_batch(ctx, cfg, cases, max_fixed, fkw, akw, sensor=False, mprior=False, stride=None, frames=None, expect=None):
    import torch
    B = len(cases)
    if frames is None:
        frames = ops.AlignFrames(0, B, stride or max_fixed, max(len(c["xyz"]) for c in cases))
        frames.max_fixed = max_fixed
        for b, c in enumerate(cases):
            frames.upload(b, c["fixed"], c["dfix"], c["xyz"], c["scale"], c["dmov"], c["X0"])
        if mprior:
            frames.prior_mean = torch.from_numpy(np.stack([c["X0"].reshape(16) for c in cases]).astype(np.float32)).cuda()
    fp, ap = _device_params(cfg, fkw, akw, sensor, mprior)
    if expect is not None:  # what the library plans for these inputs on this device (host only)
        assert ops.align_plan(fp, ap, frames.descriptor(), ops.dispatch_env(ctx))["kernels"] == expect
    ops.align_batch(ctx, fp, ap, frames)
    torch.cuda.synchronize()
    return frames


def _f64_step(cfg, c, X, corr, mean_disparity, akw, sensor=False, mprior=False):
    """float64 Gauss-Newton step (translation, rotation norms) at the device's final pose on its final correspondences"""
    cam, al = cfg["camera"], dict(cfg["aligner"])
    al.update(akw)
    P = dict(factor_type=int(al["factor_type"]), fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], cols=cam["cols"], rows=cam["rows"],
             b_lr_x=-cam["fx"] * cam.get("baseline_m", 0.0), info=al["diagonal_info"], chi_threshold=al["chi_threshold"],
             weighting=int(al["enable_inverse_depth_weighting"]), mean_disparity=float(mean_disparity))
    X = np.asarray(X, np.float64).reshape(4, 4)
    A = np.linalg.inv(SENSOR.astype(np.float64)) @ X if sensor else X  # (points -> camera)
    H, b, _, _ = rp.linearize_f64(P, A, corr, c["fixed"], c["xyz"], c["scale"])
    if mprior:  # the prior slice as the aligner adds it: diagonal information on t2tnq(Z^-1 X)
        e = rp.t2tnq(np.linalg.inv(c["X0"].astype(np.float64)) @ X)
        H = H + np.diag(MPRIOR_INFO)
        b = b + np.asarray(MPRIOR_INFO) * e
    step = rp.t2tnq(np.linalg.inv(A) @ rp.gn_step_f64(H, b, float(al["damping"]), A))
    return float(np.linalg.norm(step[:3])), float(np.linalg.norm(step[3:]))


def _check_frame(frames, b, of, res, rcorr, what):
    gcorr = frames.corr_of(b)
    assert corr_equal(rcorr, gcorr), "%s: %d vs %d correspondences" % (what, len(rcorr), len(gcorr))
    assert np.array_equal(_bits(np.array(res.X)), _bits(frames.X[b].cpu().numpy())), "%s: pose bits" % what
    gres, st = frames.result_of(b), frames.state_of(b)
    assert (gres.status, gres.warnings, gres.num_inliers, gres.num_correspondences) == (res.status, res.warnings, res.num_inliers, res.num_correspondences), what
    assert int(st.search_radius_pixels) == of.search_radius and bool(st.has_converged) == of.has_converged, what
    assert np.float32(st.descriptor_distance) == np.float32(of.descriptor_distance), what
    return gcorr, gres


def _row_parity(oracle, ctx, row, cases, cfg, stride=None):
    """the row's batch against the per-frame oracle + the float64 fixed-point check; returns (n_corr list, converged frames)"""
    fkw, akw, sensor, mprior = row.get("fkw", {}), row.get("akw", {}), bool(row.get("sensor")), bool(row.get("mprior"))
    frames = _run_batch(ctx, cfg, cases, row["max_fixed"], fkw, akw, sensor, mprior, stride=stride, expect=row_kernels(row))
    n_corr, converged = [], 0
    for b, c in enumerate(cases):
        of, res, rcorr = _oracle_frame(oracle, cfg, c, fkw, akw, sensor, mprior)
        gcorr, gres = _check_frame(frames, b, of, res, rcorr, "%s frame %d" % (row["id"], b))
        n_corr.append(len(gcorr))
        if of.has_converged and res.status == 1 and len(gcorr) >= 10:
            dt, dr = _f64_step(cfg, c, frames.X[b].cpu().numpy(), gcorr, gres.mean_disparity, akw, sensor, mprior)
            assert dt < F64_STEP_TOL and dr < F64_STEP_TOL, "%s frame %d: float64 step %.3g m / %.3g" % (row["id"], b, dt, dr)
            converged += 1
    return n_corr, converged


@pytest.mark.parametrize("row", DISPATCH, ids=[r["id"] for r in DISPATCH])
def test_every_instantiation_matches_the_oracle_and_a_float64_fixed_point(oracle, monkeypatch, row):
    cfg, cases = _cases(row["cfg"], 7100 + 13 * DISPATCH.index(row), FRAMES_PER_ROW, row["max_fixed"], full=1)
    for c in cases:
        c["scale"] = oracle.info_scale_from_nopt(c["n_opt"])
        if row.get("sensor"):
            c["X0"] = (SENSOR.astype(np.float64) @ c["X0"]).astype(np.float32)  # the robot pose whose camera is the usual guess
    ctx = _context(monkeypatch, no_lone=row["no_lone"], fused=row.get("fused", 0))
    try:
        n_corr, converged = _row_parity(oracle, ctx, row, cases, cfg)
    finally:
        ctx.close()
    assert max(n_corr) > 100, n_corr  # real correspondence sets, not empty frames
    assert converged >= FRAMES_PER_ROW // 2, "only %d converged frames to check in float64" % converged


def test_lone_threshold_both_sides(oracle, monkeypatch):
    """batch = 2 * CUs frames takes the lone instantiation, 2 * CUs + 1 the throughput one: replicas of 5 small distinct frames,
    every distinct frame against the oracle, every replica against its source frame"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    cfg, uniq = _cases("kitti", 8800, 5, 256, n_kp=300)
    for c in uniq:
        c["scale"] = oracle.info_scale_from_nopt(c["n_opt"])
    ctx = _context(monkeypatch)
    try:
        assert ops.dispatch_env(ctx).cus == n_cu
        for B, gn in ((2 * n_cu, GN("4, 4, false, 4, 1, 1")), (2 * n_cu + 1, GN("4, 4, false, 4, 4, 1"))):  # the plan flips
            cases = [uniq[b % len(uniq)] for b in range(B)]
            frames = _run_batch(ctx, cfg, cases, 256, {}, {}, expect=[AK("512, true, 2, 8"), gn])
            for u, c in enumerate(uniq):
                of, res, rcorr = _oracle_frame(oracle, cfg, c, {}, {})
                _check_frame(frames, u, of, res, rcorr, "batch %d frame %d" % (B, u))
            X, n = _bits(frames.X.cpu().numpy()), frames.n_corr.cpu().numpy()
            src = np.arange(B) % len(uniq)
            assert np.array_equal(X, X[src]) and np.array_equal(n, n[src]), "batch %d: a replica differs from its source frame" % B
            for b in range(len(uniq), B, 37):
                assert corr_equal(frames.corr_of(b), frames.corr_of(b % len(uniq))), "batch %d replica %d" % (B, b)
    finally:
        ctx.close()


# ---- capacity edges

# frames whose final correspondence count lands on the LDS-parked-row boundaries of the SLOTS = 8 instantiations: 448 rows parked by
# the five-wave one (gn_kernel<8, stereo, false, 3, 5, ..>), 576 by the lone one (and the depth / generic ones); (wanted count,
# keypoints, local-map points, fixed points kept) of make_align_case("kitti", 5000, ..), found with the oracle
EDGE_FRAMES = {
    "five": (1, [(447, 1300, 2600, 720), (448, 1300, 2600, 722), (449, 1300, 2600, 723)]),
    "lone8": (0, [(575, 1600, 3200, 927), (576, 1600, 3200, 931), (577, 1600, 3200, 932)]),
}


@pytest.mark.parametrize("which", sorted(EDGE_FRAMES))
def test_correspondence_counts_across_the_parked_row_boundary(oracle, monkeypatch, which):
    no_lone, spec = EDGE_FRAMES[which]
    cfg = configs.get("kitti")
    cases = []
    for want, n_kp, n_mv, keep in spec:
        _, fixed, dfix, mp, T, X0 = make_align_case("kitti", 5000, n_kp, n_mv)
        cases.append(dict(fixed=fixed[:keep], dfix=dfix[:keep], xyz=mp["xyz"], dmov=mp["desc"], scale=oracle.info_scale_from_nopt(mp["n_opt"]), X0=X0))
    ctx = _context(monkeypatch, no_lone=no_lone)
    try:
        n_corr, _ = _row_parity(oracle, ctx, dict(id="edge_" + which, max_fixed=1024), cases, cfg)
    finally:
        ctx.close()
    assert n_corr == [w for w, _, _, _ in spec], n_corr  # the edge cannot drift away silently


# the largest max_fixed whose fused-kernel LDS carve fits 160 KiB on the KITTI canvas (radius 50): exactly 163840 bytes
FUSED_LIMIT = 1891


@pytest.mark.parametrize("max_fixed", [512, 513, 1024, 1025, FUSED_LIMIT])
def test_max_fixed_edges_with_a_full_frame(oracle, monkeypatch, max_fixed):
    """slot change (512/513), split vs fused (1024/1025), the largest bound the fused kernel's LDS holds; two frames hold exactly
    max_fixed points"""
    cfg, cases = _cases("kitti", 9100 + max_fixed, 4 if max_fixed > 1100 else FRAMES_PER_ROW, max_fixed, full=2)
    for c in cases:
        c["scale"] = oracle.info_scale_from_nopt(c["n_opt"])
    assert len(cases[0]["fixed"]) == len(cases[1]["fixed"]) == max_fixed
    ctx = _context(monkeypatch)
    try:
        n_corr, _ = _row_parity(oracle, ctx, dict(id="max_fixed %d" % max_fixed, max_fixed=max_fixed), cases, cfg)
    finally:
        ctx.close()
    assert max(n_corr) > 100, n_corr


@pytest.mark.parametrize("max_fixed", [FUSED_LIMIT + 1, 2047, 2048])
def test_max_fixed_beyond_the_lds_or_the_class_code_is_refused(hip_ctx, max_fixed):
    """one point more than the fused kernel's LDS holds, and 2048 (the class-count code's unit), are refused before any launch"""
    cfg, cases = _cases("kitti", 9300, 1, 600)
    frames = ops.AlignFrames(0, 1, max_fixed, len(cases[0]["xyz"]))
    c = cases[0]
    frames.upload(0, c["fixed"], c["dfix"], c["xyz"], None, c["dmov"], c["X0"])
    fp, ap = _device_params(cfg, {}, {})
    with pytest.raises(ops.ProslamHipError) as ei:
        ops.align_batch(hip_ctx, fp, ap, frames)
    assert ei.value.status == ops._lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("fused", [0, 1])
def test_frame_over_its_max_fixed_fails_alone(oracle, monkeypatch, fused):
    """a frame with more fixed points than max_fixed gets PRS_ERR_CAPACITY (in result.warnings); the other frames of the batch are
    still oracle-exact"""
    cfg, cases = _cases("kitti", 9400, FRAMES_PER_ROW, 512)
    for c in cases:
        c["scale"] = oracle.info_scale_from_nopt(c["n_opt"])
    _, fixed, dfix, mp, T, X0 = make_align_case("kitti", 9499, 1000, 1000)
    assert len(fixed) > 600
    cases[2] = dict(fixed=fixed[:600], dfix=dfix[:600], xyz=mp["xyz"], dmov=mp["desc"], scale=oracle.info_scale_from_nopt(mp["n_opt"]), X0=X0)
    ctx = _context(monkeypatch, fused=fused)
    try:
        frames = _run_batch(ctx, cfg, cases, 512, {}, {}, stride=600)
        assert frames.result_of(2).warnings == ops._lib.ERR_CAPACITY
        for b, c in enumerate(cases):
            if b != 2:
                of, res, rcorr = _oracle_frame(oracle, cfg, c, {}, {})
                _check_frame(frames, b, of, res, rcorr, "frame %d" % b)
    finally:
        ctx.close()


# ---- the pruned scan's worst case and its fallback

def _correlated_frame(rng, cfg, n, corner):
    """a crowded stereo frame: n keypoints on a jittered grid, few distinct descriptors with small bit flips (correlated rows), the
    local map = the same points shuffled with descriptors 0..90 bits away.  corner: the grid ends in the canvas' last pixel, so that
    the last database entry sits in the last lattice cell a search scans"""
    cam = cfg["camera"]
    gx, gy = np.meshgrid(np.arange(28), np.arange(25))
    span = np.array([27 * 18, 24 * 12])
    origin = np.array([cam["cols"] - 1, cam["rows"] - 1]) - span if corner else np.array([300, 40])
    uv = (np.stack([gx.ravel() * 18, gy.ravel() * 12], axis=1) + origin).astype(np.float32)[-n:]
    uv += rng.integers(-3, 1 if corner else 4, uv.shape).astype(np.float32)
    if corner:
        uv[-1] = (cam["cols"] - 1, cam["rows"] - 1)
    depth = rng.uniform(6.0, 40.0, n).astype(np.float32)
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    xyz = np.stack([(uv[:, 0] - cx) / fx * depth, (uv[:, 1] - cy) / fy * depth, depth], axis=1).astype(np.float32)
    disparity = (fx * cam["baseline_m"] / depth).astype(np.float32)
    fixed = np.concatenate([uv, uv - np.stack([disparity, np.zeros(n, np.float32)], axis=1)], axis=1).astype(np.float32)
    base = syn.random_descriptors(rng, 40)
    dfix = base[rng.integers(0, 40, n)].copy()

    def flip(d, counts):
        for i in range(len(d)):
            for bit in rng.choice(256, counts[i], replace=False):
                d[i, bit // 8] ^= np.uint8(1 << (bit % 8))
    flip(dfix, rng.integers(0, 12, n))
    order = rng.permutation(n)
    dmov = dfix[order].copy()
    flip(dmov, rng.choice([0, 3, 8, 12, 16, 20, 24, 28, 31, 32, 33, 40, 48, 52, 53, 54, 55, 60, 75, 90], n))
    X0 = syn.perturb(rng, np.eye(4), 0.02, 0.001)
    return dict(fixed=fixed, dfix=dfix, xyz=xyz[order].copy(), dmov=dmov, scale=None, X0=X0)


@pytest.mark.parametrize("search_type", [1, 2, 3])
def test_full_frame_last_entry_in_last_scanned_cell(oracle, monkeypatch, search_type):
    """nF == max_fixed, the last database entry in the canvas' last lattice cell, correlated rows: the pruned scan reads one entry past
    a segment (the db[nF] sentinel) and de-duplicates survivors; split pipeline and fused kernel, both against the oracle"""
    cfg = configs.get("kitti")
    rng = np.random.default_rng(600 + search_type)
    cases = [_correlated_frame(rng, cfg, 700, corner=True) for _ in range(FRAMES_PER_ROW)]
    for c in cases:  # the corner point is in the canvas' last lattice cell and in view of the initial guess
        assert tuple(c["fixed"][-1, :2]) == (cfg["camera"]["cols"] - 1, cfg["camera"]["rows"] - 1)
    fkw = dict(search_type=search_type, maximum_search_radius_pixels=100)
    for fused in (0, 1):
        ctx = _context(monkeypatch, fused=fused)
        try:
            frames = _run_batch(ctx, cfg, cases, 700, fkw, {})
            total = 0
            for b, c in enumerate(cases):
                of, res, rcorr = _oracle_frame(oracle, cfg, c, fkw, {})
                _check_frame(frames, b, of, res, rcorr, "fused %d frame %d" % (fused, b))
                total += len(rcorr)
        finally:
            ctx.close()
        assert total > 300


RESERVED = ops.PcfState.reserved.offset
CONFIG_CHANGED = ops.PcfState.config_changed.offset


def _state_i32(frames, b, off):
    return int(frames.state[b, off:off + 4].cpu().numpy().view(np.int32)[0])


def _set_state_i32(frames, b, off, v):
    import torch
    frames.state[b, off:off + 4] = torch.from_numpy(np.array([v], np.int32).view(np.uint8).copy()).to(frames.state.device)


@pytest.mark.parametrize("fused", [0, 1])
def test_prune_fallback_switches_on_stays_exact_and_config_change_clears_it(oracle, monkeypatch, fused):
    """correlated rows overflow the survivor slots of more than an eighth of the queries: the finder stops pruning (reserved bit 0).
    Every call before and after the switch equals the oracle and the same sequence without the prefilter; the bit survives frames
    that do not overflow, and a configuration change clears it.  The caller's bits 1-31 of the word are left alone."""
    cfg = configs.get("kitti")
    rng = np.random.default_rng(4321 + fused)
    seq = [_correlated_frame(rng, cfg, 600, corner=False) for _ in range(5)]
    fkw = dict(search_type=2, maximum_search_radius_pixels=100)
    upper = 0x5A5A0000
    runs = {}
    for no_pre in (0, 1):
        ctx = _context(monkeypatch, fused=fused, no_prefilter=no_pre)
        frames = None
        try:
            of = None
            bits, outs = [], []
            for call, c in enumerate(seq):
                if frames is None:
                    frames = ops.AlignFrames(0, 1, 600, 600)
                    frames.max_fixed = 600
                    _set_state_i32(frames, 0, RESERVED, upper)
                frames.upload(0, c["fixed"], c["dfix"], c["xyz"], None, c["dmov"], c["X0"])
                frames.inputs_changed.fill_(1)
                _run_batch(ctx, cfg, [c], 600, fkw, {}, frames=frames)
                of, res, rcorr = _oracle_frame(oracle, cfg, c, fkw, {}, of=of)
                _check_frame(frames, 0, of, res, rcorr, "no_prefilter %d call %d" % (no_pre, call))
                word = _state_i32(frames, 0, RESERVED)
                assert word & ~1 == upper, "call %d: reserved 0x%x" % (call, word)
                bits.append(word & 1)
                outs.append((_bits(frames.X[0].cpu().numpy()).copy(), frames.corr_of(0).copy()))
            runs[no_pre] = outs
            if not no_pre:
                assert bits[-1] == 1, bits  # the fallback fired (the state started at 0)
                # a frame that overflows nothing keeps the hint; a configuration change clears it
                _, fixed, dfix, mp, T, X0 = make_align_case("kitti", 4400, 500, 500)
                plain = dict(fixed=fixed[:600], dfix=dfix[:600], xyz=mp["xyz"], dmov=mp["desc"], scale=None, X0=X0)
                frames.upload(0, plain["fixed"], plain["dfix"], plain["xyz"], None, plain["dmov"], plain["X0"])
                _run_batch(ctx, cfg, [plain], 600, fkw, {}, frames=frames)
                assert _state_i32(frames, 0, RESERVED) & 1 == 1
                _set_state_i32(frames, 0, CONFIG_CHANGED, 1)
                frames.upload(0, plain["fixed"], plain["dfix"], plain["xyz"], None, plain["dmov"], plain["X0"])
                _run_batch(ctx, cfg, [plain], 600, fkw, {}, frames=frames)
                assert _state_i32(frames, 0, RESERVED) == upper
        finally:
            ctx.close()
    for call, (a, b) in enumerate(zip(runs[0], runs[1])):
        assert np.array_equal(a[0], b[0]) and corr_equal(a[1], b[1]), "call %d differs from the unpruned run" % call
