"""The query cache of the split pipeline's search kernel (csrc/align.hip): a query's pruned scan leaves the cell rectangle it covered
and the survivors of the bound it kept; a later search of the same frame loop whose rectangle for that query lies inside the cached
one settles the query from its entry (a hit) and scans nothing, the others go through a queue and are scanned (misses).

Every case runs the batch four ways and compares them bit for bit: the reuse path, PRS_NO_SEARCH_REUSE=1, the fused kernel
(PRS_FUSED_ALIGN=1: everything in LDS, no cache) and the CPU checker.  Compared: correspondences in order incl. response bits, pose
bits, finder state (radius, distance, iteration, number of searches, latch, both transforms), status / warnings / counts, mean
disparity -- not the prune hint in `reserved`, which counts overflowed queries and changes no result.  Every case also asserts
through the read-out (Context.search_reuse: hits and misses of the later searches, summed over the batch) that the path it is about
actually ran.  The shapes are the smallest the path exists at: about 600 keypoints, max_fixed 600 (four survivor slots on the KITTI
canvas), at most a dozen frames."""
import numpy as np
import pytest

from helpers import make_align_case
from srrg2_proslam_amd import configs, ops
from test_align_dispatch_gpu import (CONFIG_CHANGED, RESERVED, _bits, _check_frame, _context, _correlated_frame, _device_params, _oracle_frame, _run_batch,
                                     _set_state_i32)

pytestmark = pytest.mark.gpu

MAX_FIXED = 600  # four survivor slots per thread on the KITTI canvas (660 and more: eight)


def _case(oracle, cfg_name, seed, n_kp, keep=None, sigma_t=0.05, sigma_r=0.003, n_moving=None):
    cfg, fixed, dfix, mp, T, X0 = make_align_case(cfg_name, seed, n_kp, n_moving or n_kp, sigma_t=sigma_t, sigma_r=sigma_r)
    keep = len(fixed) if keep is None else keep
    assert len(fixed) >= keep
    return dict(fixed=fixed[:keep].copy(), dfix=dfix[:keep].copy(), xyz=mp["xyz"], dmov=mp["desc"], scale=oracle.info_scale_from_nopt(mp["n_opt"]), X0=X0)


def _snapshot(frames):
    """everything a frame loop leaves behind, as comparable values (not the prune hint in `reserved`)"""
    out = []
    for b in range(frames.batch):
        n = int(frames.n_corr[b].item())
        st, res = frames.state_of(b), frames.result_of(b)
        out.append(dict(
            corr=frames.corr[b, :n].cpu().numpy().copy(),  # (fixed index, moving index, response bits) in order
            X=_bits(frames.X[b].cpu().numpy()).copy(),
            state=(int(st.search_radius_pixels), int(st.current_iteration), _bits([st.descriptor_distance]).tolist(), st.has_converged, st.config_changed,
                   st.num_recomputes, _bits(list(st.local_map_in_sensor)).tolist(), _bits(list(st.local_map_in_sensor_previous)).tolist()),
            result=(res.status, res.warnings, res.num_inliers, res.num_outliers, res.num_invalid, res.num_correspondences, res.iterations,
                    _bits([res.mean_disparity]).tolist())))
    return out


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["corr"], w["corr"]), "%s frame %d: correspondences (%d vs %d)" % (what, b, len(g["corr"]), len(w["corr"]))
        assert np.array_equal(g["X"], w["X"]), "%s frame %d: pose bits" % (what, b)
        assert g["state"] == w["state"], "%s frame %d: finder state %s vs %s" % (what, b, g["state"][:6], w["state"][:6])
        assert g["result"] == w["result"], "%s frame %d: result %s vs %s" % (what, b, g["result"], w["result"])


def _against_oracle(oracle, cfg, frames, cases, fkw, what):
    searches = []
    for b, c in enumerate(cases):
        of, res, rcorr = _oracle_frame(oracle, cfg, c, fkw, {})
        _check_frame(frames, b, of, res, rcorr, "%s frame %d" % (what, b))
        assert frames.state_of(b).num_recomputes == of.num_recomputes, "%s frame %d: number of searches" % (what, b)
        searches.append(of.num_recomputes)
    return searches


def _ctx(monkeypatch, fused=0, no_prefilter=0, no_reuse=0):
    if no_reuse:
        monkeypatch.setenv("PRS_NO_SEARCH_REUSE", "1")
    else:
        monkeypatch.delenv("PRS_NO_SEARCH_REUSE", raising=False)
    return _context(monkeypatch, fused=fused, no_prefilter=no_prefilter)


def _four_ways(oracle, monkeypatch, cfg, cases, max_fixed, fkw, what, no_prefilter=0, slots=4):
    """-> (snapshot, searches per frame, (hits, misses)) of the reuse path, after comparing it with the checker, with
    PRS_NO_SEARCH_REUSE=1 and with the fused kernel (both of which must report no hit and no miss)"""
    ctx = _ctx(monkeypatch, no_prefilter=no_prefilter)
    try:
        assert ops.dispatch_env(ctx).no_search_reuse == 0
        frames = _run_batch(ctx, cfg, cases, max_fixed, fkw, {})
        fp, ap = _device_params(cfg, fkw, {})
        assert ops.align_plan(fp, ap, frames.descriptor(), ops.dispatch_env(ctx))["surv_slots"] == slots
        searches = _against_oracle(oracle, cfg, frames, cases, fkw, what)
        reuse, counts = _snapshot(frames), ctx.search_reuse()
        for b, snap in enumerate(reuse):
            snap["hint"] = int(frames.state_of(b).reserved) & 1  # (the prune hint as the reuse path left it: for the cases that are about it, never compared)
    finally:
        ctx.close()
    for name, kw in (("no reuse", dict(no_reuse=1)), ("fused", dict(fused=1))):
        ctx = _ctx(monkeypatch, no_prefilter=no_prefilter, **kw)
        try:
            assert ops.dispatch_env(ctx).no_search_reuse == kw.get("no_reuse", 0)
            other = _snapshot(_run_batch(ctx, cfg, cases, max_fixed, fkw, {}))
            assert ctx.search_reuse() == (0, 0), name
        finally:
            ctx.close()
        _assert_same(reuse, other, "%s: reuse vs %s" % (what, name))
    print("%s: searches %s hits %d misses %d" % (what, searches, counts[0], counts[1]))
    return reuse, searches, counts


def _rectangles(cfg, c, X, radius):
    """the cell rectangle (cx0, cx1, cy0, cy1) the search scans for every moving point under pose X, and who is visible: the kernel's
    projection, clamps and 16-px cells restated in float32 numpy"""
    pr = cam = cfg["camera"]
    X = np.asarray(X, np.float32).reshape(4, 4)
    p = c["xyz"][:, :3].astype(np.float32)
    q = ((X[:3, 0] * p[:, :1] + X[:3, 1] * p[:, 1:2]) + X[:3, 2] * p[:, 2:3]) + X[:3, 3]
    z = q[:, 2]
    with np.errstate(all="ignore"):
        u = (np.float32(pr["fx"]) * q[:, 0] + np.float32(pr["cx"]) * z) / z
        v = (np.float32(pr["fy"]) * q[:, 1] + np.float32(pr["cy"]) * z) / z
    cols, rows = cam["cols"], cam["rows"]
    visible = (z >= np.float32(cfg["projector"]["range_min"])) & (z <= np.float32(cfg["projector"]["range_max"])) & (u >= 0) & (u < cols) & (v >= 0) & (v < rows)
    col, row = np.rint(np.where(visible, u, 0)).astype(np.int64), np.rint(np.where(visible, v, 0)).astype(np.int64)
    ncx = (cols + 15) >> 4
    cb0, cb1 = np.maximum(col - radius, 0), np.minimum(col + radius, (ncx << 4) - 1)
    r0, r1 = np.maximum(row - radius, 0), np.minimum(row + radius, rows - 1)
    clamped = (col - radius < 0) | (col + radius > (ncx << 4) - 1) | (row - radius < 0) | (row + radius > rows - 1)
    return np.stack([cb0 >> 4, cb1 >> 4, r0 >> 4, r1 >> 4], axis=1), visible, clamped


# ---- 1. both paths in one launch

def test_good_and_poor_start_poses_in_one_batch(oracle, monkeypatch):
    """frames that start next to their pose (the later searches move a pixel or two: hits) beside frames that start far from it (the
    second search's rectangles have left the first one's: misses)"""
    cfg = configs.get("kitti")
    cases = [_case(oracle, "kitti", 6100, 1200, keep=MAX_FIXED, n_moving=700)] + [_case(oracle, "kitti", 6100 + b, 600, n_moving=700) for b in range(1, 5)]
    cases += [_case(oracle, "kitti", 6200 + b, 600, sigma_t=0.3, sigma_r=0.02, n_moving=700) for b in range(4)]
    cases = [c if len(c["fixed"]) <= MAX_FIXED else dict(c, fixed=c["fixed"][:MAX_FIXED], dfix=c["dfix"][:MAX_FIXED]) for c in cases]
    reuse, searches, (hits, misses) = _four_ways(oracle, monkeypatch, cfg, cases, MAX_FIXED, {}, "mixed starts")
    assert min(searches) >= 2 and hits > 0 and misses > 0, (searches, hits, misses)
    assert max(len(s["corr"]) for s in reuse) > 100


def _exact_frame(rng, cfg, n):
    """a stereo frame whose measurements ARE the projections of its local map under the identity: keypoints on whole pixels, points
    un-projected from them at a random depth, the disparity unrounded, descriptors 0 .. 20 bits away from their match.  The aligner
    has nothing to correct at the true pose (float32 rounding of the points: 1e-4 px)"""
    cam = cfg["camera"]
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    cells = rng.choice(((cam["cols"] - 40) // 6) * ((cam["rows"] - 20) // 6), n, replace=False)
    per_row = (cam["cols"] - 40) // 6
    uv = np.stack([20 + 6 * (cells % per_row) + rng.integers(0, 3, n), 10 + 6 * (cells // per_row) + rng.integers(0, 3, n)], axis=1).astype(np.float32)
    depth = rng.uniform(6.0, 40.0, n).astype(np.float32)
    xyz = np.stack([(uv[:, 0] - cx) / fx * depth, (uv[:, 1] - cy) / fy * depth, depth], axis=1).astype(np.float32)
    disparity = (fx * cam["baseline_m"] / depth).astype(np.float32)
    fixed = np.concatenate([uv, uv - np.stack([disparity, np.zeros(n, np.float32)], axis=1)], axis=1).astype(np.float32)
    dfix = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    order = rng.permutation(n)
    dmov = dfix[order].copy()
    for i in range(n):
        for bit in rng.choice(256, rng.integers(0, 21), replace=False):
            dmov[i, bit // 8] ^= np.uint8(1 << (bit % 8))
    return dict(fixed=fixed, dfix=dfix, xyz=xyz[order].copy(), dmov=dmov, scale=None, X0=np.eye(4, dtype=np.float32))


def test_a_frame_that_starts_at_its_pose_only_hits(oracle, monkeypatch):
    """start pose = the true pose of measurements that are exact, and start pose = the pose the aligner converges to on a frame with
    rounded keypoints: the pose does not move, the later searches find every visible query's rectangle inside the one the first
    search scanned.  (The generated KITTI-shaped frames round their keypoints to pixels: from THEIR true pose the aligner moves by a
    fraction of a pixel to its own optimum, and the few queries next to a cell border are scanned again: 1980 hits, 6 misses.)"""
    cfg = configs.get("kitti")
    exact = _exact_frame(np.random.default_rng(6300), cfg, 480)
    _, fixed, dfix, mp, T, X0 = make_align_case("kitti", 6300, 600, 700)
    rounded = dict(fixed=fixed[:MAX_FIXED].copy(), dfix=dfix[:MAX_FIXED].copy(), xyz=mp["xyz"], dmov=mp["desc"], scale=oracle.info_scale_from_nopt(mp["n_opt"]), X0=T.copy())
    _, res, _ = _oracle_frame(oracle, cfg, rounded, {}, {})
    at_fixed_point = dict(rounded, X0=np.array(res.X, np.float32).reshape(4, 4))
    for what, c in (("start at the true pose", exact), ("start at the converged pose", at_fixed_point)):
        reuse, searches, (hits, misses) = _four_ways(oracle, monkeypatch, cfg, [c], MAX_FIXED, {}, what)
        assert searches[0] >= 2 and hits > 0 and misses == 0, (what, searches, hits, misses)
        assert len(reuse[0]["corr"]) > 100


# ---- 2. cell-border crossings

def test_pose_steps_that_move_queries_across_cell_borders(oracle, monkeypatch):
    """two frames whose pose moves by tens of pixels between the first and the last search: queries cross 16-px cell borders in each
    direction, also where the rectangle is clamped at the image border, and queries enter and leave the image (their entries go
    invalid while they are outside).  The crossings are counted here from the start pose and the final pose."""
    cfg = configs.get("kitti")
    cases = [_case(oracle, "kitti", 6400 + b, 600, keep=None, sigma_t=0.25, sigma_r=0.015, n_moving=700) for b in range(2)]
    cases = [c if len(c["fixed"]) <= MAX_FIXED else dict(c, fixed=c["fixed"][:MAX_FIXED], dfix=c["dfix"][:MAX_FIXED]) for c in cases]
    reuse, searches, (hits, misses) = _four_ways(oracle, monkeypatch, cfg, cases, MAX_FIXED, {}, "border crossings")
    radius = int(cfg["projective_finder"]["maximum_search_radius_pixels"])
    grew = shrank = at_border = entered = left = 0
    for b, c in enumerate(cases):
        first, vis0, clamp0 = _rectangles(cfg, c, c["X0"], radius)
        last, vis1, clamp1 = _rectangles(cfg, c, reuse[b]["X"].view(np.float32), radius)
        both = vis0 & vis1
        lower = (last[:, [0, 2]] < first[:, [0, 2]]).any(axis=1) & both   # a rectangle edge moved to a lower cell ...
        higher = (last[:, [1, 3]] > first[:, [1, 3]]).any(axis=1) & both  # ... to a higher one
        grew += int(lower.sum())
        shrank += int(higher.sum())
        at_border += int(((lower | higher) & (clamp0 | clamp1)).sum())
        entered += int((~vis0 & vis1).sum())
        left += int((vis0 & ~vis1).sum())
    print("crossings: lower %d higher %d at the border clamp %d entered %d left %d" % (grew, shrank, at_border, entered, left))
    assert min(grew, shrank, at_border) > 0 and entered + left > 0
    assert min(searches) >= 3 and hits > 0 and misses > 0, (searches, hits, misses)


def _search_poses(oracle, cfg, c):
    """the pose each projective search of the frame loop runs at, from the checker: a run cut after k aligner iterations tells how
    many searches k iterations hold and the pose they leave; search s runs at the start of the first iteration that counts it,
    with the pose the iterations before it left (the first one with the start pose)"""
    of, _, _ = _oracle_frame(oracle, cfg, c, {}, {})
    total, poses, X = of.num_recomputes, [], np.asarray(c["X0"], np.float32).reshape(4, 4)
    for k in range(1, 200):
        of, res, _ = _oracle_frame(oracle, cfg, c, {}, dict(max_iterations=k))
        if of.num_recomputes > len(poses):
            assert of.num_recomputes == len(poses) + 1
            poses.append(X)
        X = np.array(res.X, np.float32).reshape(4, 4)
        if len(poses) == total:
            return poses
    raise AssertionError("the checker's searches were not found in 200 iterations")


PLANTED = 6


def _plant_queries(rng, cfg, c, poses):
    """the frame with PLANTED moving points added behind its own: points that are visible in the first search, outside the image in the
    second and visible again in the third (placed a few pixels outside an image edge as the second search sees them, kept when
    the checker's poses put them in - out - in).  Their descriptors are random, 128 +- 8 bits from every row: they never survive
    the bound, never get a correspondence and so leave the frame's poses as they are.  -> (case, visibility per search of the
    planted points, the same case with the planted points behind the camera for good)"""
    cam = cfg["camera"]
    n = 100000
    edge, along, off, depth = rng.integers(0, 4, n), rng.uniform(0.05, 0.95, n), rng.uniform(0.02, 4.0, n), rng.uniform(6.0, 40.0, n)
    u = np.where(edge == 0, -off, np.where(edge == 1, cam["cols"] - 0.01 + off, along * cam["cols"]))
    v = np.where(edge == 2, -off, np.where(edge == 3, cam["rows"] - 0.01 + off, along * cam["rows"]))
    in_camera = np.stack([(u - cam["cx"]) / cam["fx"] * depth, (v - cam["cy"]) / cam["fy"] * depth, depth, np.ones(n)], axis=1)
    xyz = (np.linalg.inv(poses[1].astype(np.float64)) @ in_camera.T).T[:, :3].astype(np.float32)
    radius = int(cfg["projective_finder"]["maximum_search_radius_pixels"])
    seen = np.stack([_rectangles(cfg, dict(xyz=xyz), X, radius)[1] for X in poses], axis=1)
    pick = np.flatnonzero(seen[:, 0] & ~seen[:, 1] & seen[:, 2])[:PLANTED]
    assert len(pick) == PLANTED, "only %d candidates are in - out - in" % len(pick)
    own = np.asarray(c["xyz"], np.float32)
    add = np.zeros((PLANTED, own.shape[1]), np.float32)
    add[:, :3] = xyz[pick]
    away = add.copy()
    away[:, :3] = (0.0, 0.0, -1000.0)
    scale = c["scale"] if c["scale"] is None or np.ndim(c["scale"]) == 0 else np.concatenate([c["scale"], np.repeat(c["scale"][-1:], PLANTED, axis=0)])
    dmov = np.concatenate([c["dmov"], rng.integers(0, 256, (PLANTED, c["dmov"].shape[1])).astype(np.uint8)])
    planted = dict(c, xyz=np.concatenate([own, add]), dmov=dmov, scale=scale)
    return planted, seen[pick], dict(planted, xyz=np.concatenate([own, away]))


def _simulate(cfg, c, poses, first):
    """hits and misses of the moving points from index `first` on over the later searches, by the cache's rules: an entry is written by
    a scan (these points keep no survivor: never an overflow), dropped when the point is not visible, and serves a search whose
    rectangle lies inside it"""
    radius = int(cfg["projective_finder"]["maximum_search_radius_pixels"])
    geo = [_rectangles(cfg, dict(xyz=c["xyz"][first:]), X, radius) for X in poses]
    hits = misses = 0
    for i in range(len(c["xyz"]) - first):
        entry = None
        for s, (rect, visible, _) in enumerate(geo):
            r = rect[i]
            if not visible[i]:
                entry = None
            elif s > 0 and entry is not None and r[0] >= entry[0] and r[1] <= entry[1] and r[2] >= entry[2] and r[3] <= entry[3]:
                hits += 1
            else:
                misses += s > 0
                entry = r
    return hits, misses


def test_a_query_that_leaves_the_image_and_returns_is_scanned_again(oracle, monkeypatch):
    """visible -> invisible -> visible: the entry a query's first scan left is dropped by the search that does not see it, and the
    search that sees it again scans it although its rectangle lies inside the one the dropped entry covered (a miss, where an entry
    that had survived would give a hit).  The sequence is asserted from the checker's per-search poses; that the entries went
    invalid is read from the counts: against the same batch with the planted points out of view for good, the planted points
    add exactly the hits and misses the cache's rules give them"""
    cfg = configs.get("kitti")
    cases, controls, want_hits, want_misses = [], [], 0, 0
    for seed in (6402, 6404):
        c = _case(oracle, "kitti", seed, 600, sigma_t=0.25, sigma_r=0.015, n_moving=700)
        c = c if len(c["fixed"]) <= MAX_FIXED else dict(c, fixed=c["fixed"][:MAX_FIXED], dfix=c["dfix"][:MAX_FIXED])
        poses = _search_poses(oracle, cfg, c)
        assert len(poses) >= 3
        planted, seen, control = _plant_queries(np.random.default_rng(seed), cfg, c, poses)
        assert seen[:, 0].all() and not seen[:, 1].any() and seen[:, 2].all()
        assert [np.array_equal(a, b) for a, b in zip(poses, _search_poses(oracle, cfg, planted))] == [True] * len(poses), "the planted points moved the poses"
        h, m = _simulate(cfg, planted, poses, len(c["xyz"]))
        # by the rules every planted point is scanned in the third search; with entries that survive the second search they would all hit there
        assert m >= PLANTED
        want_hits, want_misses = want_hits + h, want_misses + m
        cases.append(planted)
        controls.append(control)
    with_points, searches, (hits, misses) = _four_ways(oracle, monkeypatch, cfg, cases, MAX_FIXED, {}, "in - out - in")
    without, _, (hits0, misses0) = _four_ways(oracle, monkeypatch, cfg, controls, MAX_FIXED, {}, "in - out - in, control")
    _assert_same(with_points, without, "planted points in view vs out of view")
    print("planted points: hits %d misses %d, by the rules %d / %d" % (hits - hits0, misses - misses0, want_hits, want_misses))
    assert (hits - hits0, misses - misses0) == (want_hits, want_misses)


# ---- 3. overflow and unpruned paths

def test_overflowed_queries_are_rescanned_and_unpruned_searches_never_hit(oracle, monkeypatch):
    """correlated rows: queries overflow their four slots, their entries are invalid and they are scanned again in every search; with
    PRS_NO_PREFILTER=1, and for a finder that arrives with the no-prune hint set, no search reads the cache"""
    cfg = configs.get("kitti")
    rng = np.random.default_rng(6500)
    cases = [_case(oracle, "kitti", 6500 + b, 1000, keep=560 + b, n_moving=700) for b in range(3)] + [_correlated_frame(rng, cfg, 600, corner=False) for _ in range(3)]
    fkw = dict(search_type=2, maximum_search_radius_pixels=100)
    pruned, _, (hits, misses) = _four_ways(oracle, monkeypatch, cfg, cases, MAX_FIXED, fkw, "correlated rows")
    assert hits > 0 and misses > 0, (hits, misses)
    # the correlated frames alone, at a radius where a few queries in a hundred meet more than four survivors: 40 distinct rows over 600
    # points on an 18 x 12 px grid, a radius of 40 px scans at most 7 x 7 cells = 112 x 112 px = 58 points, 1.5 rows of a query's kind
    # on average, five or more for about 2 % of the queries (Poisson) -- well under the eighth that would end the pruning (at 60 px the
    # window holds 96 points and the share comes to about a tenth: one frame in three latches).  The hint stays unset, every later
    # search reads the cache, and the queries that overflowed are among its misses
    alone, searches, (hits, misses) = _four_ways(oracle, monkeypatch, cfg, cases[3:], MAX_FIXED, dict(search_type=2, maximum_search_radius_pixels=40), "correlated rows alone")
    assert [snap["hint"] for snap in alone] == [0, 0, 0] and min(searches) >= 2 and hits > 0 and misses > 0, (searches, hits, misses)
    unpruned, searches, counts = _four_ways(oracle, monkeypatch, cfg, cases, MAX_FIXED, fkw, "correlated rows, no prefilter", no_prefilter=1)
    assert counts == (0, 0) and min(searches) >= 2
    _assert_same(pruned, unpruned, "pruned vs unpruned")
    # the hint set on arrival: the finder does not prune, nothing is cached
    ctx = _ctx(monkeypatch)
    try:
        frames = ops.AlignFrames(0, len(cases), MAX_FIXED, max(len(c["xyz"]) for c in cases))
        frames.max_fixed = MAX_FIXED
        for b, c in enumerate(cases):
            frames.upload(b, c["fixed"], c["dfix"], c["xyz"], c["scale"], c["dmov"], c["X0"])
            _set_state_i32(frames, b, RESERVED, 1)
            _set_state_i32(frames, b, CONFIG_CHANGED, 0)  # (a configuration change would clear the hint)
        hinted = _snapshot(_run_batch(ctx, cfg, cases, MAX_FIXED, fkw, {}, frames=frames))
        assert ctx.search_reuse() == (0, 0)
    finally:
        ctx.close()
    _assert_same(pruned, hinted, "pruned vs hinted")


# ---- 4. fixed-cloud edges, 5. pattern paths

@pytest.mark.parametrize("search_type", [1, 2, 3], ids=["square", "circle", "rhombus"])
def test_tiny_and_full_fixed_clouds_every_lattice_pattern(oracle, monkeypatch, search_type):
    """0, 1, 15, 16, 17 and exactly max_fixed fixed points in one batch, one full frame with its last lattice entry in the last cell a
    search scans; square, circle and rhombus all take the path"""
    cfg = configs.get("kitti")
    rng = np.random.default_rng(6600 + search_type)
    small = (0, 1, 15, 16, 17)
    cases = [_case(oracle, "kitti", 6600 + k, 600, keep=k, n_moving=700) for k in small]
    cases.append(_case(oracle, "kitti", 6650, 1200, keep=MAX_FIXED, n_moving=700))
    corner = _correlated_frame(rng, cfg, MAX_FIXED, corner=True)
    assert tuple(corner["fixed"][-1, :2]) == (cfg["camera"]["cols"] - 1, cfg["camera"]["rows"] - 1)
    cases.append(corner)
    fkw = dict(search_type=search_type, maximum_search_radius_pixels=100)
    reuse, searches, (hits, misses) = _four_ways(oracle, monkeypatch, cfg, cases, MAX_FIXED, fkw, "pattern %d" % search_type)
    assert [len(c["fixed"]) for c in cases] == list(small) + [MAX_FIXED, MAX_FIXED]
    assert min(searches) >= 2 and hits > 0, (searches, hits, misses)
    assert len(reuse[5]["corr"]) > 100


def test_kdtree_and_eight_slot_shapes_keep_their_path(oracle, monkeypatch):
    """the KD-tree finder and an eight-slot shape (tum.conf's parameters, 512 fixed points) report no hit and no miss"""
    cfg = configs.get("kitti")
    cases = [_case(oracle, "kitti", 6700 + b, 600, keep=380 + b, n_moving=700) for b in range(4)]
    _, searches, counts = _four_ways(oracle, monkeypatch, cfg, cases, MAX_FIXED, dict(search_type=0), "kdtree")
    assert counts == (0, 0) and min(searches) >= 2
    cfg = configs.get("tum")
    cases = [_case(oracle, "tum", 6750 + b, 600) for b in range(4)]
    cases = [c if len(c["fixed"]) <= 512 else dict(c, fixed=c["fixed"][:512], dfix=c["dfix"][:512]) for c in cases]
    _, searches, counts = _four_ways(oracle, monkeypatch, cfg, cases, 512, {}, "tum, eight slots", slots=8)
    assert counts == (0, 0) and min(searches) >= 2


# ---- 6. five and more rounds

def test_the_cache_carries_through_the_rounds_finish_adds(oracle, monkeypatch):
    """frames that need a fifth and a sixth search (launched by align_batch_finish) next to frames that are done after four"""
    cfg = configs.get("kitti")
    cases = [_case(oracle, "kitti", seed, 600, sigma_t=0.3, sigma_r=0.02, n_moving=700) for seed in range(9700, 9712)]
    cases = [c if len(c["fixed"]) <= MAX_FIXED else dict(c, fixed=c["fixed"][:MAX_FIXED], dfix=c["dfix"][:MAX_FIXED]) for c in cases]
    _, searches, (hits, misses) = _four_ways(oracle, monkeypatch, cfg, cases, MAX_FIXED, {}, "five and more rounds")
    assert searches.count(4) >= 2 and sum(n >= 6 for n in searches) >= 1 and sum(n >= 5 for n in searches) >= 3, searches
    assert hits > 0 and misses > 0


# ---- 7. context re-use

def test_one_context_other_clouds_other_strides_and_carried_finder_state(oracle, monkeypatch):
    """one context, five batches in the same buffers: other clouds in the same shape, another max_fixed and moving stride (another
    stride of the cache and of the queues), then two calls on ONE frame set whose finders carry their latched radius / distance from
    call to call (another bound: entries of the call before would be wrong, and none may be read)"""
    cfg = configs.get("kitti")
    batches = [([_case(oracle, "kitti", 6800 + b, 900, keep=500 + b, n_moving=700) for b in range(5)], 600),
               ([_case(oracle, "kitti", 6850 + b, 900, keep=520 - 7 * b, n_moving=700) for b in range(5)], 600),
               ([_case(oracle, "kitti", 6900 + b, 600, keep=300 + 11 * b, n_moving=520) for b in range(7)], 560),
               ([_case(oracle, "kitti", 6950 + b, 1500, keep=880 + b, n_moving=900) for b in range(3)], 896)]
    carried = [[_case(oracle, "kitti", 7000 + 10 * call + b, 1000, keep=540 + b, n_moving=700) for b in range(4)] for call in range(2)]

    def run(ctx, check):
        out, counts = [], []
        for i, (cases, max_fixed) in enumerate(batches):
            frames = _run_batch(ctx, cfg, cases, max_fixed, {}, {})
            if check:
                _against_oracle(oracle, cfg, frames, cases, {}, "batch %d" % i)
            out.append(_snapshot(frames))
            counts.append(ctx.search_reuse())
        frames, finders = None, [None] * 4
        for call, cases in enumerate(carried):
            if frames is None:
                frames = ops.AlignFrames(0, 4, MAX_FIXED, 700)
                frames.max_fixed = MAX_FIXED
            for b, c in enumerate(cases):
                frames.upload(b, c["fixed"], c["dfix"], c["xyz"], c["scale"], c["dmov"], c["X0"])
            frames.inputs_changed.fill_(1)
            _run_batch(ctx, cfg, cases, MAX_FIXED, {}, {}, frames=frames)
            if check:
                for b, c in enumerate(cases):
                    finders[b], res, rcorr = _oracle_frame(oracle, cfg, c, {}, {}, of=finders[b])
                    _check_frame(frames, b, finders[b], res, rcorr, "carried call %d frame %d" % (call, b))
            out.append(_snapshot(frames))
            counts.append(ctx.search_reuse())
        return out, counts

    ctx = _ctx(monkeypatch)
    try:
        reuse, counts = run(ctx, True)
    finally:
        ctx.close()
    print("hits / misses by batch:", counts)
    assert all(h > 0 for h, _ in counts), counts
    radius0 = int(cfg["projective_finder"]["maximum_search_radius_pixels"])
    assert any(s["state"][0] != radius0 for s in reuse[4]), "no finder latched: the second carried call starts with the first one's bound"
    for name, kw in (("no reuse", dict(no_reuse=1)), ("fused", dict(fused=1))):
        ctx = _ctx(monkeypatch, **kw)
        try:
            other, zero = run(ctx, False)
        finally:
            ctx.close()
        assert all(c == (0, 0) for c in zero), name
        for i, (a, b) in enumerate(zip(reuse, other)):
            _assert_same(a, b, "batch %d: reuse vs %s" % (i, name))


# ---- 8. graph replay

def test_captured_graph_replayed_on_inputs_overwritten_in_place(oracle, monkeypatch):
    """the enqueue captured in a graph and replayed twice on other frames written into the same buffers: the first search of every
    replay writes the frame's entries anew, nothing of the capture pass or of the replay before is read"""
    import torch
    cfg = configs.get("kitti")
    fp, ap = _device_params(cfg, {}, {})
    sets = [[_case(oracle, "kitti", 7100 + 50 * s + b, 1000, keep=560 + 3 * b + 5 * s, n_moving=700) for b in range(6)] for s in range(3)]

    def load(frames, cases):
        frames.reset_state()
        frames.inputs_changed.fill_(1)
        for b, c in enumerate(cases):
            frames.upload(b, c["fixed"], c["dfix"], c["xyz"], c["scale"], c["dmov"], c["X0"])

    ctx = _ctx(monkeypatch)
    try:
        frames = ops.AlignFrames(0, 6, MAX_FIXED, 700)
        frames.max_fixed = MAX_FIXED
        load(frames, sets[0])
        ops.align_batch(ctx, fp, ap, frames)  # (the scratch buffers exist from here on: nothing is allocated during the capture)
        torch.cuda.synchronize()
        _against_oracle(oracle, cfg, frames, sets[0], {}, "plain call")
        assert ctx.search_reuse()[0] > 0
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            load(frames, sets[0])
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.use_torch_stream()
                ops.align_batch_enqueue(ctx, fp, ap, frames, rounds=5)
            side.synchronize()
            ops.align_batch_finish(ctx)
            got = []
            for s in (1, 2):
                load(frames, sets[s])
                side.synchronize()
                graph.replay()
                ops.align_batch_rearm(ctx)
                ops.align_batch_finish(ctx)
                side.synchronize()
                _against_oracle(oracle, cfg, frames, sets[s], {}, "replay %d" % s)
                assert ctx.search_reuse()[0] > 0, "replay %d" % s
                got.append(_snapshot(frames))
    finally:
        ctx.close()
    for name, kw in (("no reuse", dict(no_reuse=1)), ("fused", dict(fused=1))):
        ctx = _ctx(monkeypatch, **kw)
        try:
            for s in (1, 2):
                _assert_same(got[s - 1], _snapshot(_run_batch(ctx, cfg, sets[s], MAX_FIXED, {}, {})), "replay %d: reuse vs %s" % (s, name))
        finally:
            ctx.close()
