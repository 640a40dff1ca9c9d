"""The distances in the query cache of the split pipeline's search kernel (csrc/align.hip): a query's pruned scan leaves, per distinct
survivor of the bound, its lattice position AND its full 256-bit distance in the query's entry; a later search that hits the entry
takes best and second best from those distances and reads no descriptor row.

Every case plants rows so that it exercises what it names, checks on the CPU (the checker's poses per search, the kernel's
projection, pattern and lattice restated in numpy) that the planted configuration does what the case says, and then compares four
runs bit for bit as tests/test_search_reuse_gpu.py does: the reuse path, PRS_NO_SEARCH_REUSE=1, the fused kernel and the CPU
checker (correspondences in order with response bits, pose bits, finder state and result), and asserts through
Context.search_reuse() that hits occurred.

The scenes are exact: keypoints on whole pixels, the local map un-projected from them, the true pose the identity.  The start pose
is off by TX along x (a query of depth z starts fx * TX / z pixels right of its match), so the first search runs at the start pose
and every later one within a fraction of a pixel of the identity: what a later search sees is known by construction.  kitti.conf:
circle pattern, radius 50 px, descriptor distance 25, ratio 0.8 -> the bound is 31 on the first 96 bits."""
import copy

import numpy as np
import pytest

from srrg2_proslam_amd import configs
from test_align_dispatch_gpu import _oracle_frame
from test_search_reuse_gpu import MAX_FIXED, _four_ways, _rectangles, _search_poses

pytestmark = pytest.mark.gpu

TX = 0.08     # metres the start pose is off along x
RADIUS = 50   # kitti.conf's search radius, constant until a finder converges
BOUND = 31    # irrelevant_distance(25, 0.8)


def _flipped(desc, bits):
    d = desc.copy()
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def _hamming(a, b, bits=256):
    return int(np.unpackbits(np.bitwise_xor(a, b)[:bits // 8]).sum())


class _Scene:
    """fixed points (left pixel, depth -> right pixel, descriptor) and moving points (un-projected pixel, descriptor), by hand"""

    def __init__(self, cfg, seed):
        self.cfg, self.rng = cfg, np.random.default_rng(seed)
        self.fixed, self.dfix, self.xyz, self.dmov = [], [], [], []

    def descriptor(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def fixed_point(self, u, v, desc, depth=20.0):
        cam = self.cfg["camera"]
        self.fixed.append((u, v, u - cam["fx"] * cam["baseline_m"] / depth, v))
        self.dfix.append(desc)
        return len(self.fixed) - 1

    def moving_point(self, u, v, depth, desc):
        cam = self.cfg["camera"]
        self.xyz.append(((u - cam["cx"]) / cam["fx"] * depth, (v - cam["cy"]) / cam["fy"] * depth, depth))
        self.dmov.append(desc)
        return len(self.xyz) - 1

    def pair(self, u, v, depth, dfix, dmov):
        """a fixed point and the moving point that projects onto it under the identity -> (fixed index, moving index)"""
        return self.fixed_point(u, v, dfix, depth), self.moving_point(u, v, depth, dmov)

    def background(self, n, keep=lambda u, v: True, margin_u=20):
        """n pairs on whole pixels of a jittered 6-px grid wherever keep(u, v), descriptors 0 .. 20 bits from their match"""
        cam = self.cfg["camera"]
        per_row, rows = (cam["cols"] - 2 * margin_u) // 6, (cam["rows"] - 20) // 6
        added = 0
        for cell in self.rng.permutation(per_row * rows):
            u = margin_u + 6 * int(cell % per_row) + int(self.rng.integers(0, 3))
            v = 10 + 6 * int(cell // per_row) + int(self.rng.integers(0, 3))
            if not keep(u, v):
                continue
            d = self.descriptor()
            self.pair(u, v, float(self.rng.uniform(6.0, 40.0)), d, _flipped(d, self.rng.choice(256, int(self.rng.integers(0, 21)), replace=False)))
            added += 1
            if added == n:
                return
        raise AssertionError("only %d of %d background points fit" % (added, n))

    def case(self, X0):
        assert len(self.fixed) <= MAX_FIXED
        return dict(fixed=np.array(self.fixed, np.float32), dfix=np.array(self.dfix, np.uint8), xyz=np.array(self.xyz, np.float32),
                    dmov=np.array(self.dmov, np.uint8), scale=None, X0=np.asarray(X0, np.float32))


def _shifted():
    X0 = np.eye(4, dtype=np.float32)
    X0[0, 3] = TX
    return X0


def _depth_for_shift(cfg, pixels):
    return cfg["camera"]["fx"] * TX / pixels


def _away_from(u0, v0, du=70, dv=70):
    return lambda u, v: abs(u - u0) > du or abs(v - v0) > dv


def _pixels(cfg, xyz, X):
    """(row, col) the search kernel rounds a moving point's projection to under pose X (float32, as the kernel evaluates it)"""
    cam = cfg["camera"]
    X = np.asarray(X, np.float32).reshape(4, 4)
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    q = ((X[:3, 0] * p[:, :1] + X[:3, 1] * p[:, 1:2]) + X[:3, 2] * p[:, 2:3]) + X[:3, 3]
    u = (np.float32(cam["fx"]) * q[:, 0] + np.float32(cam["cx"]) * q[:, 2]) / q[:, 2]
    v = (np.float32(cam["fy"]) * q[:, 1] + np.float32(cam["cy"]) * q[:, 2]) / q[:, 2]
    return np.rint(v).astype(np.int64), np.rint(u).astype(np.int64)


def _in_circle(row, col, fixed_row, fixed_col):
    return (fixed_col - col) ** 2 + (fixed_row - row) ** 2 <= RADIUS ** 2


def _by_the_rules(cfg, c, poses):
    """(hits, misses) [search][query] by the cache's rules: an entry is written by a scan (no query here keeps more than four
    survivors), dropped when the query is not visible, and serves a later search whose rectangle lies inside it; a hit leaves the
    entry as it is.  Also the rectangles per search"""
    geo = [_rectangles(cfg, c, X, RADIUS) for X in poses]
    n = len(c["xyz"])
    hits, misses, entry = np.zeros((len(poses), n), bool), np.zeros((len(poses), n), bool), [None] * n
    for s, (rect, visible, _) in enumerate(geo):
        for i in range(n):
            r = rect[i]
            if not visible[i]:
                entry[i] = None
            elif s > 0 and entry[i] is not None and r[0] >= entry[i][0] and r[1] <= entry[i][1] and r[2] >= entry[i][2] and r[3] <= entry[i][3]:
                hits[s, i] = True
            else:
                misses[s, i] = s > 0
                entry[i] = r
    return hits, misses, [g[0] for g in geo]


def _lattice(cfg, fixed):
    """the kernel's lattice: fixed points bucketed by 16 x 16 px cell in cell-major order (the order inside a cell is not specified)
    -> (cell of every point, point at every lattice position, first position of every cell, cells per row)"""
    cam = cfg["camera"]
    ncx, ncy = (cam["cols"] + 15) >> 4, (cam["rows"] + 15) >> 4
    col, row = fixed[:, 0].astype(np.int64), fixed[:, 1].astype(np.int64)
    cell = (row >> 4) * ncx + np.minimum(col >> 4, ncx - 1)
    order = np.argsort(cell, kind="stable")
    return cell, order, np.searchsorted(cell[order], np.arange(ncx * ncy + 1)), ncx


def _has(rcorr, fixed_idx, moving_idx, response=None):
    sel = (rcorr["fixed_idx"] == fixed_idx) & (rcorr["moving_idx"] == moving_idx)
    return bool(sel.any()) and (response is None or float(rcorr["response"][sel][0]) == float(response))


def _checked_on_the_cpu(oracle, cfg, c, query):
    """the checker's poses per search, hits and misses by the rules, the final correspondences; the planted query must be settled
    from its entry in every later search"""
    poses = _search_poses(oracle, cfg, c)
    assert len(poses) >= 3 and np.array_equal(poses[0], c["X0"])
    hits, misses, rects = _by_the_rules(cfg, c, poses)
    assert hits[1:, query].all(), "the planted query is scanned again: %s" % [r[query].tolist() for r in rects]
    _, _, rcorr = _oracle_frame(oracle, cfg, c, {}, {})
    return poses, hits, misses, rects, rcorr


def _run(oracle, monkeypatch, cfg, c, what, hits_by_rule, misses_by_rule):
    _, searches, (hits, misses) = _four_ways(oracle, monkeypatch, cfg, [c], MAX_FIXED, {}, what)
    print("%s: by the rules, per search: hits %s misses %s" % (what, hits_by_rule.sum(axis=1).tolist(), misses_by_rule.sum(axis=1).tolist()))
    assert searches[0] == len(hits_by_rule) and hits > 0
    assert (hits, misses) == (int(hits_by_rule.sum()), int(misses_by_rule.sum()))


# ---- 1. a distance recorded without ever being scored

def test_survivor_outside_the_pattern_when_cached_inside_it_at_the_hit(oracle, monkeypatch):
    """the query starts 8 px right of its match and is 4 px right of it in the second search; a fixed point 45 px left of the match
    lies 53 px from the query in the search that writes the entry (outside the circle, inside the scanned cells) and 49 px or less
    from it in every later one.  It is 2 bits from the query, the true match 10: the later searches must make it the query's best
    from a distance no search ever scored"""
    cfg = configs.get("kitti")
    sc = _Scene(cfg, 7301)
    row, col = 200, 16 * 30 + 52  # (col - 50 = 16 k + 2: the later rectangles start in the cell the first one starts in)
    dA = sc.descriptor()
    F, A = sc.pair(col, row, _depth_for_shift(cfg, 8.0), _flipped(dA, range(100, 110)), dA)
    P = sc.fixed_point(col - 45, row, _flipped(dA, (130, 131)))
    sc.background(480, _away_from(col, row))
    c = sc.case(_shifted())
    poses, hits, misses, rects, rcorr = _checked_on_the_cpu(oracle, cfg, c, A)
    assert _hamming(c["dfix"][P], dA, 96) < BOUND and _hamming(c["dfix"][P], dA) == 2 and _hamming(c["dfix"][F], dA) == 10
    r0, c0 = _pixels(cfg, c["xyz"][A], poses[0])
    assert not _in_circle(r0[0], c0[0], row, col - 45) and _in_circle(r0[0], c0[0], row, col)
    cx0, cx1, cy0, cy1 = rects[0][A]
    assert cx0 <= (col - 45) >> 4 <= cx1 and cy0 <= row >> 4 <= cy1, "the planted point is not in a cell the first search scans"
    for X in poses[1:]:
        r, cc = _pixels(cfg, c["xyz"][A], X)
        assert _in_circle(r[0], cc[0], row, col - 45) and _in_circle(r[0], cc[0], row, col)
    assert _has(rcorr, P, A, 2)
    _run(oracle, monkeypatch, cfg, c, "outside, then inside", hits, misses)


# ---- 2. four survivors, Lowe's ratio from cached distances

def test_four_cached_survivors_decide_best_second_best_and_the_ratio(oracle, monkeypatch):
    """the query's entry holds four survivors at 10, 11, 20 and 24 bits, all within 10 px of it: best and second best of every later
    search are the first two.  The filter accepts a fixed point's lowest response when it is below 0.8 of the second lowest:
      * a second query without a match of its own is 12 bits from the first one's best: that fixed point meets 10 and 12 (0.83);
      * the first query's second best has a match of its own 9 bits away and meets 9 and 11 (0.82).
    Neither gets a correspondence, and both ratios are made of distances read from entries"""
    cfg = configs.get("kitti")
    sc = _Scene(cfg, 7302)
    row, col = 184, 16 * 40 + 8
    dA = sc.descriptor()
    dF, dP1 = _flipped(dA, range(0, 10)), _flipped(dA, range(20, 31))
    F, A = sc.pair(col, row, _depth_for_shift(cfg, 5.3), dF, dA)
    P1, Q = sc.pair(col + 2, row + 4, 12.0, dP1, _flipped(dP1, range(210, 219)))
    P2 = sc.fixed_point(col - 6, row - 4, _flipped(dA, list(range(40, 50)) + list(range(130, 140))))
    P3 = sc.fixed_point(col - 2, row + 6, _flipped(dA, range(140, 164)))
    B = sc.moving_point(col + 12, row - 8, 15.0, _flipped(dF, range(200, 212)))
    sc.background(480, _away_from(col, row))
    c = sc.case(_shifted())
    poses, hits, misses, rects, rcorr = _checked_on_the_cpu(oracle, cfg, c, A)
    assert [_hamming(c["dfix"][i], dA) for i in (F, P1, P2, P3)] == [10, 11, 20, 24]
    assert _hamming(c["dfix"][F], c["dmov"][B]) == 12 and _hamming(c["dfix"][P1], c["dmov"][Q]) == 9
    for q in (A, B, Q):  # (four survivors each: nobody overflows the slots)
        survivors = [i for i in range(len(c["fixed"])) if _hamming(c["dfix"][i], c["dmov"][q], 96) < BOUND]
        assert sorted(survivors) == sorted((F, P1, P2, P3)), "query %d does not keep exactly the four planted survivors" % q
        assert min((_hamming(c["dfix"][i], c["dmov"][q]), i) for i in survivors)[1] == (P1 if q == Q else F)
        for X in poses:
            r, cc = _pixels(cfg, c["xyz"][q], X)
            assert all(_in_circle(r[0], cc[0], c["fixed"][i, 1], c["fixed"][i, 0]) for i in (F, P1, P2, P3))
    assert hits[1:, B].all() and hits[1:, Q].all()
    assert not np.isin(rcorr["fixed_idx"], (F, P1, P2, P3)).any() and not np.isin(rcorr["moving_idx"], (A, B, Q)).any()
    _run(oracle, monkeypatch, cfg, c, "four survivors", hits, misses)


# ---- 3. equal distances

def test_equal_cached_distances_are_ordered_by_canonical_position(oracle, monkeypatch):
    """three survivors 10 bits from the query, in one row of cells: X in cell k, Y one pixel row above it in cell k + 1, Z one pixel row
    below it in cell k - 1.  The canonical (row-major) order is Y, X, Z, the lattice's cell-major order Z, X, Y: best is Y, second
    best X, Z is not emitted.  X and Z have matches of their own 9 bits away: X meets 9 and the query's 10 (0.9) and gets no
    correspondence, Z meets 9 alone and gets one.  Any other order of the three moves a correspondence"""
    cfg = configs.get("kitti")
    sc = _Scene(cfg, 7303)
    row, col = 16 * 12 + 8, 16 * 35 + 8
    dA = sc.descriptor()
    dX, dZ = _flipped(dA, range(100, 110)), _flipped(dA, range(140, 150))
    X_, A = sc.pair(col, row, _depth_for_shift(cfg, 5.3), dX, dA)
    QX = sc.moving_point(col, row, 14.0, _flipped(dX, range(200, 209)))
    Y_ = sc.fixed_point(16 * 36 + 4, row - 1, _flipped(dA, range(120, 130)))
    Z_, QZ = sc.pair(16 * 34 + 12, row + 1, 16.0, dZ, _flipped(dZ, range(220, 229)))
    sc.background(480, _away_from(col, row))
    c = sc.case(_shifted())
    poses, hits, misses, rects, rcorr = _checked_on_the_cpu(oracle, cfg, c, A)
    assert [_hamming(c["dfix"][i], dA) for i in (X_, Y_, Z_)] == [10, 10, 10]
    assert _hamming(c["dfix"][X_], c["dmov"][QX]) == 9 and _hamming(c["dfix"][Z_], c["dmov"][QZ]) == 9
    cell, order, cellstart, ncx = _lattice(cfg, c["fixed"])
    assert cell[Z_] + 1 == cell[X_] == cell[Y_] - 1, "lattice order is not Z, X, Y"
    assert c["fixed"][Y_, 1] < c["fixed"][X_, 1] < c["fixed"][Z_, 1], "canonical order is not Y, X, Z"
    for X in poses:
        r, cc = _pixels(cfg, c["xyz"][A], X)
        assert all(_in_circle(r[0], cc[0], c["fixed"][i, 1], c["fixed"][i, 0]) for i in (X_, Y_, Z_))
    assert hits[1:, QX].all() and hits[1:, QZ].all()
    assert _has(rcorr, Y_, A, 10) and not (rcorr["fixed_idx"] == X_).any() and _has(rcorr, Z_, QZ, 9)
    _run(oracle, monkeypatch, cfg, c, "equal distances", hits, misses)


# ---- 4. a survivor read twice

def test_a_survivor_read_behind_one_segment_and_again_in_its_own_is_scored_once(oracle, monkeypatch):
    """the query's match is alone in its cell, nothing lies left of it in its row of cells and nothing right of the query's rectangle
    in the row of cells above, whose segment holds an odd number of entries: the scan that writes the entry reads the match as the
    entry one past that segment and again as the first of the next one.  Scored twice on a hit, it would be its own second best and
    fail the ratio test; it must keep its correspondence"""
    cfg = configs.get("kitti")
    sc = _Scene(cfg, 7304)
    kF, jF = 30, 10
    row, col = 16 * jF + 8, 16 * kF + 8
    dA = sc.descriptor()
    F, A = sc.pair(col, row, _depth_for_shift(cfg, 5.3), _flipped(dA, range(100, 107)), dA)
    cx0, cx1 = (col + 5 - RADIUS) >> 4, (col + 5 + RADIUS) >> 4  # the first search's rectangle (the query starts 5 px right)

    def keep(u, v):
        if v >> 4 == jF:
            return u >= 16 * (kF + 1)
        if v >> 4 == jF - 1:
            return u < 16 * (cx1 + 1)
        return True
    sc.background(480, keep)
    above = sum(1 for u, v, _, _ in sc.fixed if int(v) >> 4 == jF - 1 and cx0 <= int(u) >> 4 <= cx1)
    if above % 2 == 0:
        sc.fixed_point(16 * cx0 + 3, 16 * (jF - 1) + 3, sc.descriptor())
    c = sc.case(_shifted())
    poses, hits, misses, rects, rcorr = _checked_on_the_cpu(oracle, cfg, c, A)
    assert rects[0][A].tolist()[:2] == [cx0, cx1] and rects[0][A][2] <= jF - 1 and rects[0][A][3] >= jF
    cell, order, cellstart, ncx = _lattice(cfg, c["fixed"])
    seg0, seg1 = cellstart[(jF - 1) * ncx + cx0], cellstart[(jF - 1) * ncx + cx1 + 1]
    assert (seg1 - seg0) % 2 == 1, "the segment above holds an even number of entries: nothing is read past it"
    assert order[seg1] == F and cellstart[jF * ncx + cx0] == seg1, "the entry one past the segment above is not the match"
    assert (cell == cell[F]).sum() == 1
    assert _hamming(c["dfix"][F], dA, 96) < BOUND and _has(rcorr, F, A, 7)
    _run(oracle, monkeypatch, cfg, c, "read twice", hits, misses)


# ---- 5. the fields' extremes

@pytest.mark.parametrize("words", [3, 4], ids=["96 bits", "128 bits"])
def test_largest_and_smallest_distance_and_the_last_lattice_position(oracle, monkeypatch, words):
    """the query is identical to its match (distance 0), which is the last entry of a full lattice (position max_fixed - 1); a second
    survivor equals the query on the compared words and is its complement on all other bits (160 / 128: the largest full distance a
    survivor of the bound can have).  That one has a match of its own 24 bits away, whose acceptance needs 24 / 160 (24 / 128) < 0.8:
    a distance that lost its high bits in the entry would reject it.  128 bits: minimum_descriptor_distance 35, bound 43"""
    cfg = copy.deepcopy(configs.get("kitti"))
    if words == 4:
        cfg["projective_finder"]["minimum_descriptor_distance"] = 35.0
    bits = 32 * words
    cam = cfg["camera"]
    sc = _Scene(cfg, 7305 + words)
    row, col = 372, 16 * 75 + 8  # the last row of cells; nothing else lies in it
    dA = sc.descriptor()
    F, A = sc.pair(col, row, _depth_for_shift(cfg, 5.3), dA.copy(), dA)
    dP = _flipped(dA, range(bits, 256))
    P, C = sc.pair(col - 20, row - 10, 18.0, dP, _flipped(dP, range(bits, bits + 24)))
    sc.background(MAX_FIXED - 2, lambda u, v: v >> 4 < row >> 4 and (abs(u - col) > 70 or abs(v - row) > 70))
    c = sc.case(_shifted())
    assert len(c["fixed"]) == MAX_FIXED
    poses = _search_poses(oracle, cfg, c)
    assert len(poses) >= 3
    hits, misses, rects = _by_the_rules(cfg, c, poses)
    assert hits[1:, A].all() and hits[1:, C].all()
    cell, order, cellstart, ncx = _lattice(cfg, c["fixed"])
    assert order[MAX_FIXED - 1] == F and (cell == cell[F]).sum() == 1, "the match is not the last lattice entry"
    assert _hamming(dP, dA, bits) == 0 and _hamming(dP, dA) == 256 - bits and _hamming(c["dfix"][F], dA) == 0
    assert _hamming(c["dmov"][C], dP) == 24 and _hamming(c["dmov"][C], dP, bits) == 0
    _, _, rcorr = _oracle_frame(oracle, cfg, c, {}, {})
    assert _has(rcorr, F, A, 0) and _has(rcorr, P, C, 24)
    _run(oracle, monkeypatch, cfg, c, "extremes, %d bits" % bits, hits, misses)


# ---- 6. entries refreshed by a search that misses throughout

def test_a_search_that_misses_for_every_query_leaves_entries_the_next_one_hits(oracle, monkeypatch):
    """keypoints in the middle third of the image, the start pose rotated by 0.06 rad about the vertical axis: every query starts
    43 - 47 px beside its match and the aligner takes back 21 px or more of that before the second search, more than a cell.  The
    second search finds no rectangle inside the first one's, scans every query and writes every entry anew -- other rectangles,
    other survivors -- and the third search, a few pixels on, settles most queries from those"""
    cfg = configs.get("kitti")
    sc = _Scene(cfg, 7306)
    sc.background(500, margin_u=400)
    X0 = np.eye(4, dtype=np.float32)
    X0[0, 0] = X0[2, 2] = np.cos(0.06)
    X0[0, 2], X0[2, 0] = np.sin(0.06), -np.sin(0.06)
    c = sc.case(X0)
    poses = _search_poses(oracle, cfg, c)
    assert len(poses) >= 3
    hits, misses, rects = _by_the_rules(cfg, c, poses)
    n = len(c["xyz"])
    _, col0 = _pixels(cfg, c["xyz"], poses[0])
    _, col1 = _pixels(cfg, c["xyz"], poses[1])
    assert (np.abs(col1 - col0) > 16).all()
    assert hits[1].sum() == 0 and misses[1].sum() == n, "the second search does not miss throughout"
    assert hits[2].sum() > n // 2, "the third search does not hit the refreshed entries"
    # (entries the first search wrote would serve none of them: every hit of the third search is on an entry the second one wrote)
    assert not any((r2 >= r0)[[0, 2]].all() and (r2 <= r0)[[1, 3]].all() for r0, r2 in zip(rects[0], rects[2]))
    _, _, rcorr = _oracle_frame(oracle, cfg, c, {}, {})
    assert len(rcorr) > 400
    _run(oracle, monkeypatch, cfg, c, "refreshed entries", hits, misses)
