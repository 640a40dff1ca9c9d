"""CPU restatement of the loop detector's candidate search (include/proslam_hip.h, prs_place_*; csrc/place_db.hip).

`Database.query` restates CorrespondenceFinderHBST_::compute (correspondence_finder_hbst.cpp:5-91, :95-127) around an EXHAUSTIVE
database match: the Valid filter, index_query, the uint64_t age rule, the strict inlier rule, candidates in ascending map index and,
per candidate, the best query point of every matched reference descriptor (the earlier query point on a tie).  The distances come
from one float32 matrix product per map (exact: integers <= 256).  `query_loop` is the independent check: a direct pairwise loop in
the reference's own shape (matches in query order, an unordered map of candidates keyed by reference descriptor, strict <).
"""
import numpy as np

WARN_EMPTY_INPUT, ERR_CAPACITY, ERR_RANGE = 1, -2, -4
CORR_DTYPE = np.dtype([("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])
_U64 = 1 << 64


def params(maximum_descriptor_distance=25.0, minimum_age_difference_to_candidates=0, relocalize_min_inliers=0, max_candidates=8):
    return dict(maximum_descriptor_distance=maximum_descriptor_distance,
                minimum_age_difference_to_candidates=minimum_age_difference_to_candidates,
                relocalize_min_inliers=relocalize_min_inliers, max_candidates=max_candidates)


def _bits(desc):
    return np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)


def distances(q_desc, r_desc):
    """[nq, nr] Hamming distances (int64)"""
    a, b = _bits(q_desc), _bits(r_desc)
    if not len(a) or not len(b):
        return np.zeros((len(a), len(b)), np.int64)
    d = a.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (a @ b.T)
    return np.rint(d).astype(np.int64)


def age_ok(index_query, reference, minimum_age):
    """std::fabs(index_query - entry.first) > minimum_age_difference_to_candidates with uint64_t operands"""
    return float((index_query - reference) % _U64) > float(minimum_age)


def inliers_ok(count, min_inliers):
    """number_of_matches (size_t) > relocalize_min_inliers: a negative value compares as a huge unsigned one"""
    return min_inliers >= 0 and count > min_inliers


class Database:
    """what prs_place_db holds: per map its graph id, Valid descriptors (and xyz) in point order, their point indices"""

    def __init__(self):
        self.maps = []

    def add(self, graph_id, desc, valid=None, xyz=None):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        assert graph_id >= 0 and all(m["graph_id"] != graph_id for m in self.maps)
        keep = np.arange(len(desc)) if valid is None else np.flatnonzero(np.asarray(valid) != 0)
        xyz = np.zeros((len(desc), 3), np.float32) if xyz is None else np.asarray(xyz, np.float32).reshape(-1, 3)
        self.maps.append(dict(graph_id=graph_id, desc=desc[keep], pidx=keep.astype(np.int32), xyz=xyz[keep]))
        return len(self.maps) - 1

    def index_query(self, graph_id):
        for i, m in enumerate(self.maps):
            if m["graph_id"] == graph_id:
                return i
        return len(self.maps)

    def query(self, P, graph_id, desc, valid=None):
        """-> dict(status, index_query, counts [maps], candidates [<= max_candidates], corr [list of CORR_DTYPE arrays])"""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        iq = self.index_query(graph_id)
        out = dict(status=0, index_query=iq, counts=np.zeros(len(self.maps), np.int64), candidates=[], corr=[])
        if graph_id < 0:
            out["status"] = ERR_RANGE
            return out
        if n == 0:
            out["status"] = WARN_EMPTY_INPUT
            return out
        qv = np.arange(n) if valid is None else np.flatnonzero(np.asarray(valid) != 0)
        thr = np.float32(P["maximum_descriptor_distance"])
        best = []
        for m in self.maps:
            d = distances(desc[qv], m["desc"])
            hit = d.astype(np.float32) < thr
            best.append((d, hit))
        out["counts"] = np.array([h.sum() for _, h in best], np.int64)
        passing = [i for i in range(len(self.maps))
                   if age_ok(iq, i, P["minimum_age_difference_to_candidates"]) and inliers_ok(out["counts"][i], P["relocalize_min_inliers"])]
        if len(passing) > P["max_candidates"]:
            out["status"] = ERR_CAPACITY
        for i in passing[: P["max_candidates"]]:
            d, hit = best[i]
            cols = np.flatnonzero(hit.any(0))
            rows = []
            for c in cols:
                dc = np.where(hit[:, c], d[:, c], 1 << 20)
                k = int(np.argmin(dc))  # first minimum = earlier query point
                rows.append((qv[k], self.maps[i]["pidx"][c], float(d[k, c])))
            out["candidates"].append(i)
            out["corr"].append(np.array(rows, dtype=CORR_DTYPE))
        return out


def query_loop(db, P, graph_id, desc, valid=None):
    """the same query by a direct pairwise loop in the reference's shape -> (candidates, corr list, counts)"""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    if len(desc) == 0:
        return [], [], [0] * len(db.maps)
    iq = db.index_query(graph_id)
    thr = float(np.float32(P["maximum_descriptor_distance"]))
    pop = lambda x: int(np.unpackbits(x).sum())  # noqa: E731
    matches = {}
    for qi in range(len(desc)):
        if valid is not None and valid[qi] == 0:
            continue
        for mi, m in enumerate(db.maps):
            for r in range(len(m["desc"])):
                dist = pop(desc[qi] ^ m["desc"][r])
                if dist < thr:
                    matches.setdefault(mi, []).append((qi, int(m["pidx"][r]), dist))
    counts = [len(matches.get(i, [])) for i in range(len(db.maps))]
    cands, corr = [], []
    for ref in sorted(matches):
        if age_ok(iq, ref, P["minimum_age_difference_to_candidates"]) and inliers_ok(len(matches[ref]), P["relocalize_min_inliers"]):
            candidates = {}
            for qi, r, dist in matches[ref]:
                if r in candidates:
                    if dist < candidates[r][2]:
                        candidates[r] = (qi, r, dist)
                else:
                    candidates[r] = (qi, r, dist)
            cands.append(ref)
            corr.append(np.array([candidates[r] for r in sorted(candidates)], dtype=CORR_DTYPE))
    return cands[: P["max_candidates"]], corr[: P["max_candidates"]], counts


def gather_pairs(db, result, desc, xyz, valid, max_candidates):
    """what prs_place_gather_pairs promises for one query: `max_candidates` slots of dict(fixed_desc, fixed_xyz, n_fixed, moving_desc,
    moving_xyz, n_moving, X).  Slot k < len(result["candidates"]) holds the query's Valid descriptors and points in index order
    (fixed) and the stored rows of candidate k (moving); every other slot has both counts 0.  X is the identity in every slot."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    xyz = np.zeros((len(desc), 3), np.float32) if xyz is None else np.asarray(xyz, np.float32).reshape(-1, 3)
    qv = np.arange(len(desc)) if valid is None else np.flatnonzero(np.asarray(valid)[: len(desc)] != 0)
    empty = dict(fixed_desc=desc[:0], fixed_xyz=xyz[:0], n_fixed=0, moving_desc=desc[:0], moving_xyz=xyz[:0], n_moving=0)
    slots = []
    for k in range(max_candidates):
        slot = dict(empty)
        if k < len(result["candidates"]):
            m = db.maps[result["candidates"][k]]
            slot.update(fixed_desc=desc[qv], fixed_xyz=xyz[qv], n_fixed=len(qv), moving_desc=m["desc"], moving_xyz=m["xyz"],
                        n_moving=len(m["desc"]))
        slot["X"] = np.eye(4, dtype=np.float32)
        slots.append(slot)
    return slots


# ------------------------------------------------------------------------------------------------------------ scenarios
def recognition_3d(B):
    """test_place_recognition.cpp 3D cases: (name, map 0 desc, query desc, thr, min_inliers, pinned correspondence count | None)"""
    import ref_pins as rp
    k, i0, i1 = rp.kitti_fixture(B), rp.icl_measurements(B, 0), rp.icl_measurements(B, 1)
    n = len(k["desc"][0])
    return [dict(name="kitti_3d_00_00", ref=k["desc"][0], query=k["desc"][0], thr=1.0, min_inliers=n - 1, pin=n, perfect=True),
            dict(name="kitti_3d_00_01", ref=k["desc"][0], query=k["desc"][1], thr=50.0, min_inliers=50, pin=74, perfect=False),
            dict(name="icl_3d_00_01", ref=i0["desc"], query=i1["desc"], thr=50.0, min_inliers=250, pin=213, perfect=False)]


def features_2d(B, which):
    """the oracle extractor at FAST 5, target 1000, 3 x 3 bins (test_place_recognition.cpp 2D cases)"""
    import ref_pins as rp
    img = {"kitti_00": lambda: rp.kitti_image("left", 0), "kitti_01": lambda: rp.kitti_image("left", 1),
           "icl_00": lambda: rp.icl_gray(0), "icl_50": lambda: rp.icl_gray(50)}[which]()
    return B.extract(img, 5, 1000, 3, 3)[1]


def recognition_2d(B):
    f = {w: features_2d(B, w) for w in ("kitti_00", "kitti_01", "icl_00", "icl_50")}
    n = len(f["kitti_00"])
    return [dict(name="kitti_2d_00_00", ref=f["kitti_00"], query=f["kitti_00"], thr=1.0, min_inliers=n - 1, pin=n, perfect=True),
            dict(name="kitti_2d_00_01", ref=f["kitti_00"], query=f["kitti_01"], thr=25.0, min_inliers=100, pin=259, perfect=False),
            dict(name="icl_2d_00_50", ref=f["icl_00"], query=f["icl_50"], thr=25.0, min_inliers=100, pin=103, perfect=False)], f


FEATURE_PINS = {"kitti_00": 866, "kitti_01": 874, "icl_00": 538, "icl_50": 451}
