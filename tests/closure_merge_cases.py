"""Inputs of the closure-merger tests, shared by the CPU suite (which checks that every case exercises what its name says, on the
numpy rule) and the GPU suite (which compares the kernel with that rule byte for byte): the reference's ICL frames behind its two
gtests (tests/test_mergers.cpp:174-246), small synthetic pairs at the edges of the kernel's paths (EDGES) and pairs of up to 16384
measurements, a bitmap word for every thread of the kernel's workgroup (SIZES)."""
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
              corner=None, half_bins=False, landmarks_from=None, alias=0, **kw):
    """one pair.  The first n_corr measurements (shuffled) are matched to distinct landmarks: most lie within the merge distance
    of their landmark, a fifth further away, a tenth carry a response >= 50 (some exactly 50).  corner = (u0, v0, u1, v1) confines
    the image positions to that box (so that few bins are hit).  half_bins snaps the positions to the middle of every 8 x 8 px cell
    (8 k + 4): with bins of that width v / row_w and u / col_w are exact halves, where std::round and round-half-even part.
    landmarks_from = r draws the matched landmarks from rows r .. n_scene - 1 only; with alias = a a quarter of them are named
    again a rows further up (distinct landmarks whose indices agree in their low bits)."""
    rng = np.random.default_rng(seed)
    assert n_corr <= min(n_scene, n_meas)
    T = np.eye(4, dtype=f32) if transform is None else np.asarray(transform, f32)
    box = (0.0, 0.0, COLS - 1e-3, ROWS - 1e-3) if corner is None else corner
    u = rng.uniform(box[0], box[2], n_meas).astype(f32)
    v = rng.uniform(box[1], box[3], n_meas).astype(f32)
    if half_bins:
        u, v = np.floor(u / f32(8)) * f32(8) + f32(4), np.floor(v / f32(8)) * f32(8) + f32(4)
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
    mi = rng.permutation(n_meas)[:n_corr]
    if landmarks_from is None:
        si = rng.permutation(n_scene)[:n_corr]
    elif not alias:
        si = landmarks_from + rng.permutation(n_scene - landmarks_from)[:n_corr]
    else:
        k = n_corr // 4
        low = landmarks_from + rng.permutation(n_scene - alias - landmarks_from)[:k]
        rest = np.setdiff1d(np.arange(landmarks_from, n_scene), np.concatenate([low, low + alias]))
        si = rng.permutation(np.concatenate([low, low + alias, rng.permutation(rest)[:n_corr - 2 * k]]))
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


# ---- the sizes of a real map: a bitmap word for every thread of the workgroup ----------------------------------------------------
# A measurement bitmap of 16384 bits is 256 words, one per thread; wave w of the workgroup owns the words of measurements
# 4096 w .. 4096 w + 4095.  The cases below put non-zero words, caps and winners into every wave.
WAVE = 4096


def per_wave(idx):
    """how many of the measurement indices fall to each of the four waves"""
    return np.bincount(np.asarray(idx, np.int64) // WAVE, minlength=4)[:4]


def n_candidates(info, case):
    """the valid measurements that were not merged"""
    valid = cr.measurement_points(case["P"], case["measurement"])[1]
    return int(valid.sum()) - int(valid[info["merged"]].sum())


def merged_landmarks(info, case):
    """the landmarks of the correspondences whose measurement was merged (exact where no two correspondences share a measurement)"""
    a = case.get("corr_from_aligner", 0)
    m, s = case["corr"]["fixed_idx" if a else "moving_idx"], case["corr"]["moving_idx" if a else "fixed_idx"]
    return s[np.isin(m, info["merged"])]


def rint_bins_differ(info, case):
    """binned measurements whose bin would be another under round-half-even"""
    P, z = case["P"], case["measurement"]
    row_w, col_w = f32(P["canvas_rows"]) / f32(P["number_of_row_bins"]), f32(P["canvas_cols"]) / f32(P["number_of_col_bins"])
    other = np.rint(z[:, 1] / row_w).astype(np.int64) * (P["number_of_col_bins"] + 2) + np.rint(z[:, 0] / col_w).astype(np.int64)
    return int(((info["bins"] >= 0) & (info["bins"] != other)).sum())


def share_measurement(c, k0, others):
    """correspondences `others` are renamed to correspondence k0's measurement and their landmarks moved onto k0's landmark: several
    landmarks merge with ONE measurement (only landmarks must be distinct), so n_measured - n_merged undercounts the candidates"""
    a = c.get("corr_from_aligner", 0)
    m, s = c["corr"]["fixed_idx" if a else "moving_idx"], c["corr"]["moving_idx" if a else "fixed_idx"]
    m[others] = m[k0]
    for name in ("coords", "state"):
        if name in c["scene"]:
            c["scene"][name][s[others], :3] = c["scene"][name][s[k0], :3]
    return c


_BINS = dict(row_bins=60, col_bins=80)
_BIG = dict(n_scene=400, n_meas=16384)
_all_added = lambda r, i, c: (r[2] == 0 and r[1] == n_candidates(i, c) and (per_wave(i["added"]) > 0).all() and r[0] > 256 * 5)  # noqa: E731
_shared = lambda r, i, c: (r[2] == 0 and r[1] == i["n_to_add"] < n_candidates(i, c)  # noqa: E731
                           and r[0] + n_candidates(i, c) < c["P"]["target_number_of_merges"] and len(i["merged"]) < r[0])

# name -> (arguments of synthetic, predicate on (result, info, case)); "share" in the arguments is taken out by size()
SIZES = {
    "cap_in_wave_2": (dict(seed=61, **_BIG, n_corr=300, target=9000, binning=0),
                      lambda r, i, c: r[2] == 0 and i["added"][-1] // WAVE == 2 and (i["added"][-1] + 1) % 64 != 0
                      and (per_wave(i["added"])[:3] > 0).all() and per_wave(i["added"])[3] == 0),
    "winners_in_all_waves": (dict(seed=62, **_BIG, n_corr=50, target=9000, **_BINS),
                             lambda r, i, c: r[2] == 0 and (per_wave(i["pass1"]) > 0).all() and 0 < len(i["pass1"]) < r[1]
                             and (per_wave(np.setdiff1d(i["added"], i["pass1"]))[:2] > 0).all()),
    "pass1_cut_in_wave_1": (dict(seed=63, **_BIG, n_corr=50, target=1500, **_BINS),
                            lambda r, i, c: r[2] == 0 and i["n_winners"] > len(i["pass1"]) == i["n_to_add"] == r[1] and i["pass1"][-1] // WAVE == 1),
    **{"n_measured_%d" % n: (dict(seed=s, n_scene=400, n_meas=n, n_corr=50, target=4000, **_BINS),
                             lambda r, i, c, n=n: r[2] == 0 and r[1] > 0 and (n != 4097 or 4096 in i["added"]))
       for s, n in ((64, 4095), (65, 4096), (85, 4097))},  # (seed 85: measurement 4096 wins its bin, so pass 1 adds it)
    **{"n_measured_%d" % n: (dict(seed=s, n_scene=5000, n_meas=n, n_corr=5000, target=100000), _all_added) for s, n in ((67, 16383), (68, 16384))},
    # (target 12000, not 9000: pass 2 takes candidates in measurement order and has to get past wave 1)
    "xyz_16384": (dict(seed=62, **_BIG, n_corr=50, target=12000, **_BINS, kind=cr.XYZ, n_behind=2000, n_off_canvas=2000, n_invalid=64),
                  lambda r, i, c: r[2] == 0 and len(i["pass1"]) > 0
                  and (per_wave(np.setdiff1d(i["added"], i["pass1"])[i["bins"][np.setdiff1d(i["added"], i["pass1"])] < 0]) > 0).sum() >= 3),
    "from_aligner_inverse_16384": (dict(seed=61, **_BIG, n_corr=300, target=9000, binning=0, transform=_X, inverse=1, from_aligner=1),
                                   lambda r, i, c: r[2] == 0 and r[0] > 100 and r[1] > 0),
    "shared_measurement": (dict(seed=69, n_scene=300, n_meas=200, n_corr=100, target=1000, share=0), _shared),
    "shared_measurement_16384": (dict(seed=70, **_BIG, n_corr=300, target=100000, **_BINS, share=3 * WAVE),
                                 lambda r, i, c: _shared(r, i, c) and c["shared"] >= 3 * WAVE and c["shared"] in i["merged"]),
    # (bins of 8 x 8 px: 62 x 82 of them fit the kernel's 64 KiB of LDS, the 122 x 82 of 4 px rows would be refused at the call)
    "half_bins": (dict(seed=71, n_scene=100, n_meas=400, n_corr=10, target=150, row_bins=ROWS // 8, col_bins=COLS // 8, half_bins=True),
                  lambda r, i, c: r[2] == 0 and rint_bins_differ(i, c) > 100 and 0 < len(i["pass1"]) and n_candidates(i, c) > i["n_to_add"]),
    "high_landmarks": (dict(seed=72, n_scene=200000, n_meas=300, n_corr=257, target=1000, capacity=200320, landmarks_from=131072, alias=65536),
                       lambda r, i, c: r[2] == 0 and r[0] > 50 and (c["corr"]["fixed_idx"] >= 131072).sum() >= 100
                       and merged_landmarks(i, c).max() >= 131072 + 65536
                       and np.isin(merged_landmarks(i, c) + 65536, merged_landmarks(i, c)).sum() >= 20),  # both of a pair 2^16 apart
}


def size(name):
    """a case of SIZES, with the numpy rule's answer beside it (computed once: c["want"] = (scene after, result, info))"""
    key = "size_" + name
    if key not in _cache:
        args, check = SIZES[name]
        args = dict(args)
        share = args.pop("share", None)
        c = synthetic(**args)
        if share is not None:  # the first correspondence whose measurement index is >= share takes nine others' landmarks
            k0 = int(np.nonzero(c["corr"]["moving_idx"] >= share)[0][0])
            share_measurement(c, k0, [k for k in range(k0 + 1, k0 + 10)])
            c["shared"] = int(c["corr"]["moving_idx"][k0])
        c["name"], c["check"] = name, check
        c["want"] = want(c)
        _cache[key] = c
    return _cache[key]


def error_batch_sizes():
    """three pairs of one launch at full size: the first fault in vector order is a duplicate landmark (entry 16000) with a
    measurement index out of range behind it (entry 16200); the same two swapped; a good pair.  -> [(case, code)]"""
    if "errors_sizes" not in _cache:
        base = dict(n_scene=20000, n_meas=16384, n_corr=16384, target=100000)
        out = []
        c = synthetic(seed=80, **base)
        c["corr"]["fixed_idx"][16000] = c["corr"]["fixed_idx"][5]
        c["corr"]["moving_idx"][16200] = 16384
        out.append((c, cr.ERR_DUPLICATE))
        c = synthetic(seed=81, **base)
        c["corr"]["moving_idx"][16000] = 16384
        c["corr"]["fixed_idx"][16200] = c["corr"]["fixed_idx"][5]
        out.append((c, cr.ERR_RANGE))
        out.append((synthetic(seed=82, **base), cr.OK))
        for c, _ in out:
            c["want"] = want(c)
        _cache["errors_sizes"] = out
    return _cache["errors_sizes"]


def mixed_group():
    """pairs of 16384, 4097, 1 and 0 measured and cap_in_wave_2 for ONE launch: a launch has one capacity and one set of parameters,
    so all five take the group's largest capacity and the binning and target of winners_in_all_waves"""
    if "mixed" not in _cache:
        common = dict(target=9000, binning=1, **_BINS, capacity=5000 + 16384)
        out = []
        for name, args in (("n_measured_16384", SIZES["n_measured_16384"][0]), ("n_measured_4097", SIZES["n_measured_4097"][0]),
                           ("n_measured_1", dict(seed=90, n_scene=400, n_meas=1, n_corr=1)),
                           ("n_measured_0", dict(seed=91, n_scene=400, n_meas=0, n_corr=0)), ("cap_in_wave_2", SIZES["cap_in_wave_2"][0])):
            c = synthetic(**dict(args, **common))
            c["name"], c["want"] = "mixed " + name, None
            c["want"] = want(c)
            out.append(c)
        _cache["mixed"] = out
    return _cache["mixed"]
