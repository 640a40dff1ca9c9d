"""Inputs of the closure-merger tests, shared by the CPU suite (which checks that every case exercises what its name says, on the
numpy rule) and the GPU suite (which compares the kernel with that rule byte for byte): the reference's ICL frames behind its two
gtests (tests/test_mergers.cpp:174-246) and small synthetic pairs at the edges of the kernel's paths."""
import numpy as np

import closure_merge_ref as cr
import ref_mapping as rm
import ref_pins as rp

f32 = np.float32
ROWS, COLS = 480, 640
K = (481.2, -481.0, 319.5, 239.5)  # fixtures.hpp:577 (ICL)
_cache = {}


def rows4(a):
    """[n, 3] -> [n, 4] measurement / coordinate rows (fourth float 0)"""
    a = np.asarray(a, f32).reshape(-1, 3)
    return np.concatenate([a, np.zeros((len(a), 1), f32)], axis=1)


def icl(B):
    """scene = the 321 points of frame 00; measurements of 00 and 01 in both kinds; the fixture's ideal correspondences"""
    if "icl" not in _cache:
        m0, m1 = rp.icl_measurements(B, 0), rp.icl_measurements(B, 1)
        uvd = lambda m: rows4(np.concatenate([m["uv"], m["depth"][:, None]], axis=1))  # noqa: E731
        _cache["icl"] = dict(scene=cr.make_scene(512, m0["xyz"], m0["desc"]),
                             meas={("00", cr.UVD): uvd(m0), ("01", cr.UVD): uvd(m1), ("00", cr.XYZ): rows4(m0["xyz"]), ("01", cr.XYZ): rows4(m1["xyz"])},
                             desc={"00": m0["desc"], "01": m1["desc"]},
                             corr={"00": rm._identity_corr(321).astype(cr.CORR_DTYPE),
                                   "01": rm.icl_ideal_correspondences(m0, m1, rp.icl_relative(1, 0)).astype(cr.CORR_DTYPE)})
    return _cache["icl"]


# (frame, distance, target, binning) -> (points after, merged, added): the two pins of the reference and the cap at work
ICL_CASES = [("00", 0.25, 1000, 1, (321, 321, 0)), ("01", 0.25, 1000, 1, (431, 228, 110))] + [
    ("01", 0.01, t, b, w) for t, w in ((200, (321, 215, 0)), (250, (356, 215, 35)), (300, (406, 215, 85))) for b in (1, 0)]


def icl_case(B, frame, distance2, target, binning, kind=cr.UVD):
    d = icl(B)
    P = cr.params(kind=kind, enable_binning=binning, max_distance2=distance2, target=target)
    return dict(P=P, scene=d["scene"], measurement=d["meas"][(frame, kind)], measurement_desc=d["desc"][frame], corr=d["corr"][frame],
                transform=np.eye(4, dtype=f32), scene_in_world=rigid(7, 0.3, 2.0))


def rigid(seed, angle, shift):
    """a rotation by `angle` about a random axis and a translation of length <= shift, float32"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)
    T[:3, 3] = rng.uniform(-shift, shift, 3)
    return T.astype(f32)


def synthetic(seed, n_scene, n_meas, n_corr, kind=cr.UVD, capacity=None, transform=None, inverse=0, from_aligner=0, with_stats=True,
              target=200, binning=1, row_bins=10, col_bins=30, n_invalid=0, n_behind=0, n_off_canvas=0, depth_ties=False,
              corner=None, **kw):
    """one pair.  The first n_corr measurements (shuffled) are matched to distinct landmarks: most lie within the merge distance
    of their landmark, a fifth further away, a tenth carry a response >= 50 (some exactly 50).  corner = (u0, v0, u1, v1) confines
    the image positions to that box (so that few bins are hit)."""
    rng = np.random.default_rng(seed)
    assert n_corr <= min(n_scene, n_meas)
    T = np.eye(4, dtype=f32) if transform is None else np.asarray(transform, f32)
    box = (0.0, 0.0, COLS - 1e-3, ROWS - 1e-3) if corner is None else corner
    u = rng.uniform(box[0], box[2], n_meas).astype(f32)
    v = rng.uniform(box[1], box[3], n_meas).astype(f32)
    d = rng.uniform(0.5, 6.0, n_meas).astype(f32)
    if depth_ties:
        d = np.round(d).astype(f32) + f32(1)  # few distinct depths: ties inside a bin go to the lowest index
    z = rows4(np.stack([u, v, d], axis=1))
    P = cr.params(kind=cr.UVD, enable_binning=binning, row_bins=row_bins, col_bins=col_bins, rows=ROWS, cols=COLS, K=K, target=target, **kw)
    p, _ = cr.measurement_points(P, z)
    P["measurement_kind"] = kind
    special = rng.permutation(n_meas)
    if kind == cr.UVD:
        bad = [0.0, -1.0, np.nan, np.inf, -np.inf, -0.0]
        for k, i in enumerate(special[:n_invalid]):
            z[i, 2] = bad[k % len(bad)]
    else:
        z[:, :3] = p
        for k, i in enumerate(special[:n_invalid]):
            z[i, k % 3] = [np.nan, np.inf, -np.inf][k % 3]
        for k, i in enumerate(special[n_invalid:n_invalid + n_behind]):
            z[i, 2] = [0.0, -z[i, 2], -0.0][k % 3]
        for i in special[n_invalid + n_behind:n_invalid + n_behind + n_off_canvas]:
            z[i, 0] = z[i, 2] * f32(3.0) * (1 if i % 2 else -1)  # |x / z| = 3: far outside the field of view
    p, _ = cr.measurement_points(P, z)
    q = cr.apply_rows(cr.se3_inverse(T) if inverse else T, np.nan_to_num(p, nan=1.0, posinf=1.0, neginf=1.0))
    xyz = rng.uniform(-4, 4, (n_scene, 3)).astype(f32)
    mi, si = rng.permutation(n_meas)[:n_corr], rng.permutation(n_scene)[:n_corr]
    noise = rng.normal(0, 0.05, (n_corr, 3))
    noise[rng.random(n_corr) < 0.2] += 2.0
    xyz[si] = (q[mi] + noise).astype(f32)
    corr = np.zeros(n_corr, cr.CORR_DTYPE)
    corr["moving_idx" if from_aligner else "fixed_idx"] = si
    corr["fixed_idx" if from_aligner else "moving_idx"] = mi
    resp = rng.uniform(0, 49, n_corr).astype(f32)
    high = rng.random(n_corr) < 0.1
    resp[high] = np.where(rng.random(int(high.sum())) < 0.5, 50.0, 77.0)
    corr["response"] = resp
    cap = n_scene + n_meas if capacity is None else capacity
    scene = cr.make_scene(cap, xyz, rng.integers(0, 256, (n_scene, 32), dtype=np.uint8), with_stats)
    # rows past n_points, and the statistics of every row, carry a pattern: nothing may leak, nothing may be skipped
    scene["coords"][n_scene:] = -7.0
    scene["coords"][:, 3] = np.arange(cap, dtype=f32)
    scene["desc"][n_scene:] = 0xAB
    if with_stats:
        scene["state"][:] = -3.0
        scene["covariance"][:] = 9.0
        scene["n_opt"][:] = rng.integers(0, 5, cap)
        scene["inlier"][:] = 2
        scene["n_meas"][:] = 6
    return dict(P=P, scene=scene, measurement=z, measurement_desc=rng.integers(0, 256, (n_meas, 32), dtype=np.uint8), corr=corr,
                transform=T, scene_in_world=rigid(seed + 1, 0.5, 3.0) if with_stats else None,
                transform_is_scene_in_measurement=inverse, corr_from_aligner=from_aligner)


def want(case, **kw):
    """the numpy rule on a case -> (scene after, (n_merged, n_added, status), info)"""
    info = {}
    S, res = cr.closure_merge(case["P"], case["scene"], case["measurement"], case["measurement_desc"], case["corr"], case["transform"],
                              scene_in_world=case.get("scene_in_world"),
                              transform_is_scene_in_measurement=case.get("transform_is_scene_in_measurement", 0),
                              corr_from_aligner=case.get("corr_from_aligner", 0), info=info, **kw)
    return S, res, info


_X = rigid(3, 0.4, 1.5)

# name -> (arguments of synthetic, a predicate on (result, info, case) that says the case is the one its name promises)
EDGES = {
    **{"n_corr_%d" % n: (dict(seed=10 + n, n_scene=300, n_meas=300, n_corr=n, target=1000),
                         lambda r, i, c, n=n: r[2] == 0 and (n == 0 or 0 < r[0] < n or n == 1) and r[1] == 300 - r[0]) for n in (0, 1, 63, 64, 65, 257)},
    **{"n_measured_%d" % n: (dict(seed=20 + n, n_scene=80, n_meas=n, n_corr=min(n, 40), target=1000),
                             lambda r, i, c, n=n: r[2] == 0 and r[0] + r[1] == n) for n in (1, 64, 65, 300)},
    "cap_mid_wave": (dict(seed=31, n_scene=200, n_meas=300, n_corr=64, target=83, binning=0),
                     lambda r, i, c: r[1] == 83 - r[0] and r[1] % 64 != 0 and list(i["added"]) == [m for m in range(300) if m not in set(i["merged"])][:r[1]]),
    "pass1_longer_than_cap": (dict(seed=32, n_scene=200, n_meas=300, n_corr=64, target=70),
                              lambda r, i, c: i["n_winners"] > len(i["pass1"]) == i["n_to_add"] == r[1] > 0),
    "pass2_needed": (dict(seed=33, n_scene=200, n_meas=300, n_corr=4, target=150, row_bins=2, col_bins=2),
                     lambda r, i, c: 0 < len(i["pass1"]) < r[1] == i["n_to_add"]),
    "all_bins_blocked": (dict(seed=34, n_scene=200, n_meas=300, n_corr=120, target=160, row_bins=1, col_bins=1),
                         lambda r, i, c: len(i["pass1"]) == 0 and r[1] == i["n_to_add"] > 0),
    "depth_ties": (dict(seed=35, n_scene=100, n_meas=300, n_corr=20, target=60, row_bins=3, col_bins=4, depth_ties=True),
                   lambda r, i, c: 0 < len(i["pass1"]) <= r[1] == i["n_to_add"]),
    "invalid_depths": (dict(seed=36, n_scene=100, n_meas=200, n_corr=100, target=1000, n_invalid=30),
                       lambda r, i, c: r[0] + r[1] == 200 - 30),
    "xyz_unbinned": (dict(seed=37, n_scene=100, n_meas=300, n_corr=30, kind=cr.XYZ, target=120, row_bins=3, col_bins=4, n_invalid=6, n_behind=40,
                         n_off_canvas=40),
                     lambda r, i, c: r[1] == i["n_to_add"] and (i["bins"] < 0).sum() >= 80 and len(i["pass1"]) < r[1]
                     and (i["bins"][i["added"]] < 0).any()),
    "xyz_all": (dict(seed=38, n_scene=100, n_meas=128, n_corr=64, kind=cr.XYZ, target=1000), lambda r, i, c: r[0] + r[1] == 128),
    "transform": (dict(seed=39, n_scene=150, n_meas=200, n_corr=100, transform=_X, target=130), lambda r, i, c: r[0] > 50 and r[1] > 0),
    "transform_inverse": (dict(seed=39, n_scene=150, n_meas=200, n_corr=100, transform=_X, inverse=1, target=130), lambda r, i, c: r[0] > 50 and r[1] > 0),
    "from_aligner": (dict(seed=40, n_scene=150, n_meas=200, n_corr=100, transform=_X, inverse=1, from_aligner=1, target=130),
                     lambda r, i, c: r[0] > 50 and r[1] > 0),
    "no_stats": (dict(seed=41, n_scene=150, n_meas=200, n_corr=100, with_stats=False, target=130), lambda r, i, c: r[0] > 50 and r[1] > 0),
    "target_reached": (dict(seed=42, n_scene=150, n_meas=200, n_corr=100, target=10), lambda r, i, c: r[0] > 10 and r[1] == 0),
    "exactly_full": (dict(seed=43, n_scene=100, n_meas=90, n_corr=50, target=1000, capacity=None), None),  # capacity set by edge()
}


def edge(name):
    if name not in _cache:
        args, check = EDGES[name]
        c = synthetic(**args)
        if name == "exactly_full":  # n_points + n_added == capacity is accepted
            _, r, _ = want(c)
            c = synthetic(**dict(args, capacity=100 + r[1]))
            check = lambda r, i, c: r[2] == 0 and 100 + r[1] == c["scene"]["coords"].shape[0] and r[1] > 0  # noqa: E731
        c["name"], c["check"] = name, check
        _cache[name] = c
    return _cache[name]


def error_batch():
    """five pairs of one batch: PRS_ERR_RANGE, _CAPACITY, _DUPLICATE, _SCENE_FULL and a good one; + the counts to upload"""
    if "errors" not in _cache:
        base = dict(n_scene=100, n_meas=120, n_corr=60, target=1000, capacity=256)
        out = []
        c = synthetic(seed=50, **base)
        c["corr"]["moving_idx"][17] = 120  # a measurement index past the cloud; the duplicate further on must not win
        c["corr"]["fixed_idx"][40] = c["corr"]["fixed_idx"][39]
        out.append((c, {}, cr.ERR_RANGE))
        c = synthetic(seed=51, **base)
        out.append((c, dict(n_measured=129), cr.ERR_CAPACITY))  # stride of the batch: 128
        c = synthetic(seed=52, **base)
        c["corr"]["fixed_idx"][30] = c["corr"]["fixed_idx"][3]
        c["corr"]["fixed_idx"][45] = 100  # out of range AFTER the duplicate in vector order
        out.append((c, {}, cr.ERR_DUPLICATE))
        c = synthetic(seed=53, **dict(base, capacity=256))
        c["scene"]["n_points"] = 200  # rows 100 .. 199 hold the pattern; 200 + the additions exceed 256
        out.append((c, {}, cr.ERR_SCENE_FULL))
        out.append((synthetic(seed=54, **base), {}, cr.OK))
        _cache["errors"] = out
    return _cache["errors"]
