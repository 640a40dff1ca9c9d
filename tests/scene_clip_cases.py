"""Inputs of exactly known content for the scene clipper's tests (csrc/scene_clip.hip), built once per process and shared by
tests/test_scene_clip_cases.py (CPU) and tests/test_scene_clip_edges_gpu.py.

Planting rule.  A frustum edge is planted in PIXEL space at a power-of-two depth: for a pixel (u, v) and a depth z the point is
x = (u z - cx z) / fx, y = (v z - cy z) / fy with power-of-two fx, fy.  Every float32 step of the projection of such a point is
exact (checked in float64 by _plant), so the float32 rule and the float64 statement scene_clip_ref.inside agree on it and the
expected verdict is simply 0 <= u < cols, 0 <= v < rows, range_min <= z <= range_max of the planted numbers.  Stepping x by one ulp
from an edge instead does not work: fx x + cx z rounds back onto the boundary for about one point in eight.

A batch (dict): proj, S [4,4], stride, xyzw [B,stride,4], desc [B,stride,32], n_scene [B] (as handed to the kernel: may be negative
or above the stride), R [B,4,4], n_opt [B,stride] uint32, names [B].  Rows at and past n_scene hold inside points, so only the
row-count comparison keeps them out.  expected(batch, b, with_nopt) is scene_clip_ref.clip of the clamped scene, computed once.
"""
import functools
import types

import numpy as np

import scene_clip_ref as ref
from tests import helpers as hp

F = np.float32
I4 = np.eye(4, dtype=F)
TILE, SUB, WAVE = 1024, 256, 64

# fx = fy = 256 (a power of two), principal point at the canvas centre
PLANTED = dict(fx=256.0, fy=256.0, cx=320.0, cy=240.0, canvas_cols=640, canvas_rows=480, range_min=0.5, range_max=8.0)
# a tall canvas with the principal point on its left edge and range_min = 0: x = +-0 lies on u = 0 and z = +-0 reaches the division
TALL = dict(fx=64.0, fy=128.0, cx=0.0, cy=256.0, canvas_cols=96, canvas_rows=512, range_min=0.0, range_max=4.0)
PROJECTORS = {"planted": PLANTED, "tall": TALL}
DEPTHS = {"planted": (0.5, 1.0, 2.0, 4.0, 8.0), "tall": (0.25, 4.0)}

SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073, 4097)
PATTERNS = ("all", "none", "first", "last", "alt_row", "alt_wave", "alt_sub", "tile_k")
AGES = np.array([0, 1, 2, 3, 4, 4094, 4095, 4096, 2 ** 31, 2 ** 32 - 1], np.uint32)
BOUNDARY_ROWS = (63, 64, 255, 256, 1023, 1024)

INSIDE_POINT = np.array([0.25, -0.125, 2.0], F)   # pixel (352, 224) of PLANTED
OUTSIDE_POINT = np.array([8.0, -0.125, 2.0], F)   # pixel (1344, 224): only u >= cols rejects it


def projector(module, name):
    """module.Projector (oracle.binding or srrg2_proslam_amd._lib) of a named projector"""
    p = PROJECTORS[name]
    return module.Projector(p["fx"], p["fy"], p["cx"], p["cy"], p["canvas_cols"], p["canvas_rows"], p["range_min"], p["range_max"])


def plain(name):
    """the same fields without ctypes, for scene_clip_ref"""
    return types.SimpleNamespace(**PROJECTORS[name])


def signature_desc(rows, salt=0):
    """32 bytes per row that name the row: a descriptor written to the wrong slot is seen"""
    i = (np.asarray(rows, np.uint64) + np.uint64(salt) * np.uint64(1000003)).astype(np.uint32)
    words = np.stack([(i * np.uint32(2654435761) + np.uint32(k) * np.uint32(40503)) ^ (i >> np.uint32(k)) for k in range(8)], axis=-1)
    return np.ascontiguousarray(words.astype(np.uint32)).view(np.uint8).reshape(-1, 32)


def signature_w(rows):
    return (np.asarray(rows, np.int64) + 1).astype(F)  # exact in float32 for every row used here


# ------------------------------------------------------------------------------------------------------------ planted edges
def _exact32(*values):
    return all(bool(np.all(np.asarray(v, np.float64) == np.asarray(v, np.float64).astype(F).astype(np.float64))) for v in values)


def _plant(name, u, v, z):
    """the point of pixel (u, v) at depth z; asserts in float64 that every float32 step of its projection is exact"""
    p = PROJECTORS[name]
    u, v, z = float(F(u)), float(F(v)), float(F(z))
    x = (u * z - p["cx"] * z) / p["fx"]
    y = (v * z - p["cy"] * z) / p["fy"]
    hx, hy = p["fx"] * x + p["cx"] * z, p["fy"] * y + p["cy"] * z
    assert _exact32(x, y, u * z, v * z, p["cx"] * z, p["cy"] * z, p["fx"] * x, p["fy"] * y, hx, hy), (name, u, v, z)
    assert hx / z == u and hy / z == v, (name, u, v, z)
    return [x, y, z]


def pixel_values(size):
    s = F(size)
    return [F(-2.0 ** -10), F(0.0), F(2.0 ** -10), F(size / 2), np.nextafter(s, F(0)), s, np.nextafter(s, F(np.inf))]


@functools.lru_cache(maxsize=None)
def planted(name):
    """-> dict(xyz [n,3] float32, keep [n] bool (the verdict of the planted numbers), boundary [n] bool (some planted number lies on
    an edge or one ulp from it), exact [n] bool (every float32 step exact), uvz [n,3] float64)"""
    p = PROJECTORS[name]
    rows = []
    us, vs = pixel_values(p["canvas_cols"]), pixel_values(p["canvas_rows"])
    for z in DEPTHS[name]:
        for u in us:
            for v in vs:
                edge = not (u == us[3] and v == vs[3] and z not in (p["range_min"], p["range_max"]))
                rows.append((_plant(name, u, v, z), (float(u), float(v), float(z)), edge, True))
    # the depth's neighbours at the image centre: cx z is no longer exact, the pixel is the centre to within a rounding and only
    # the depth decides
    lo, hi = F(p["range_min"]), F(p["range_max"])
    near = [np.nextafter(hi, F(0)), np.nextafter(hi, F(np.inf))]
    if lo > 0:
        near += [np.nextafter(lo, F(0)), np.nextafter(lo, F(np.inf))]
    for z in near:
        zc = float(z)
        xc = (us[3] * zc - p["cx"] * zc) / p["fx"]
        assert _exact32(xc)
        rows.append(([xc, 0.0, zc], (float(us[3]), float(vs[3]), zc), True, False))
    xyz = np.array([r[0] for r in rows], np.float64)
    assert _exact32(xyz)
    uvz = np.array([r[1] for r in rows], np.float64)
    keep = ((uvz[:, 0] >= 0) & (uvz[:, 0] < p["canvas_cols"]) & (uvz[:, 1] >= 0) & (uvz[:, 1] < p["canvas_rows"])
            & (uvz[:, 2] >= p["range_min"]) & (uvz[:, 2] <= p["range_max"]))
    return dict(xyz=xyz.astype(F), keep=keep, boundary=np.array([r[2] for r in rows]), exact=np.array([r[3] for r in rows]), uvz=uvz)


@functools.lru_cache(maxsize=None)
def specials(name):
    """points outside the planting rule, compared with the float32 restatement and the C checker only.  -> (xyz [n,3], keep [n],
    what [n]).  The verdict of each is stated here by hand, following the reference's loop: a row is dropped when a comparison is
    TRUE, so a row whose depth and pixel are NaN is kept."""
    nan, inf = np.nan, np.inf
    rows = []
    if name == "planted":
        # the pose is a full matrix product: 0 * inf = NaN reaches every camera coordinate, 0 * NaN likewise -> all kept
        for k in range(3):
            for bad in (nan, inf, -inf):
                q = [0.25, -0.125, 2.0]
                q[k] = bad
                # ... except an infinite depth, which stays infinite and fails its range comparison
                rows.append((q, not (k == 2 and np.isinf(bad)), "%s in %s" % (bad, "xyz"[k])))
        rows.append(([0.25, -0.125, -2.0], False, "negative depth, pixel (352, 224) inside the canvas"))
        rows.append(([0.0, 0.0, 0.0], False, "zero depth below range_min"))
        rows.append(([-0.0, -0.0, 2.0], True, "-0.0 in x and y at the centre"))
    else:
        rows.append(([0.0, 0.0, 1.0], True, "x = +0 on u = 0"))
        # fx * (-0) + cx * z = (-0) + (+0) = +0 in round to nearest: u is +0, on the edge and inside
        rows.append(([-0.0, 0.0, 1.0], True, "x = -0 on u = 0"))
        rows.append(([-2.0 ** -149, 0.0, 1.0], False, "the smallest x below 0: u = -2^-143"))
        rows.append(([0.0, 0.0, 0.0], True, "0 / 0 = NaN pixel at z = +0 = range_min"))
        rows.append(([0.0, 0.0, -0.0], True, "0 / -0 = NaN pixel; -0 < 0 is false"))
        rows.append(([-0.0, -0.0, -0.0], True, "-0 / -0 = NaN pixel"))
        rows.append(([0.5, 0.0, 0.0], False, "u = +inf at z = +0"))
        rows.append(([0.5, 0.0, -0.0], False, "u = -inf at z = -0"))
        rows.append(([-0.5, 0.0, 0.0], False, "u = -inf at z = +0"))
        rows.append(([0.0, 0.0, -1.0], False, "negative depth, pixel (0, 256) inside the canvas"))
        rows.append(([0.0, 0.0, 2.0 ** -149], True, "the smallest depth above range_min = 0"))
    return np.array([r[0] for r in rows], F), np.array([r[1] for r in rows]), [r[2] for r in rows]


@functools.lru_cache(maxsize=None)
def edge_cloud(name):
    """the planted points and the specials of a projector shuffled into one cloud of 1300 rows: a kept boundary point at rows 63,
    255 and 1023 (the last lane of a wave, of a sub-tile, of a tile) and a dropped one at rows 64, 256 and 1024 (the first of the
    next).  -> dict(xyzw, desc, keep (stated verdict), planted_rows, planted_index, special_rows, boundary_rows)"""
    n = 1300
    rng = np.random.default_rng(41 if name == "planted" else 42)
    P, (sx, sk, _) = planted(name), specials(name)
    p = PROJECTORS[name]
    col = P["uvz"][:, 0]
    on_edge = P["exact"] & (P["uvz"][:, 1] == p["canvas_rows"] / 2) & (P["uvz"][:, 2] == DEPTHS[name][-1])
    kept_edge = int(np.flatnonzero(on_edge & (col == 0.0))[0])                       # u == 0: kept
    dropped_edge = int(np.flatnonzero(on_edge & (col == float(p["canvas_cols"])))[0])  # u == cols: dropped
    assert P["keep"][kept_edge] and not P["keep"][dropped_edge]
    total = len(P["xyz"]) + len(sx)
    free = np.setdiff1d(np.arange(n), np.array(BOUNDARY_ROWS))
    where = np.sort(rng.choice(free, total, replace=False))
    order = rng.permutation(total)
    xyz = np.zeros((n, 3), F)
    keep = np.zeros(n, bool)
    # filler: clearly inside and clearly outside points, alternating irregularly
    fill_in = rng.random(n) < 0.5
    xyz[:] = np.where(fill_in[:, None], INSIDE_POINT, OUTSIDE_POINT) if name == "planted" else \
        np.where(fill_in[:, None], np.array([0.5, 0.25, 1.0], F), np.array([4.0, 0.25, 1.0], F))
    keep[:] = fill_in
    src_xyz = np.concatenate([P["xyz"], sx])
    src_keep = np.concatenate([P["keep"], sk])
    xyz[where] = src_xyz[order]
    keep[where] = src_keep[order]
    planted_rows = where[order < len(P["xyz"])]
    planted_index = order[order < len(P["xyz"])]
    for r in BOUNDARY_ROWS:
        k = kept_edge if r % 2 else dropped_edge
        xyz[r], keep[r] = P["xyz"][k], P["keep"][k]
    rows = np.arange(n)
    xyzw = np.concatenate([xyz, signature_w(rows)[:, None]], axis=1).astype(F)
    return dict(xyzw=xyzw, desc=signature_desc(rows, 7), keep=keep, planted_rows=planted_rows, planted_index=planted_index,
                special_rows=where[order >= len(P["xyz"])], boundary_rows=BOUNDARY_ROWS)


# ------------------------------------------------------------------------------------------------------------ keep patterns
def pattern(kind, n):
    i = np.arange(n)
    if kind == "all":
        return np.ones(n, bool)
    if kind == "none":
        return np.zeros(n, bool)
    if kind == "first":
        return i == 0
    if kind == "last":
        return i == n - 1
    if kind == "alt_row":
        return i % 2 == 1
    if kind == "alt_wave":
        return (i // WAVE) % 2 == 0
    if kind == "alt_sub":
        return (i // SUB) % 2 == 1
    if kind == "tile_k":
        return i // TILE == ((n - 1) // TILE + 1) // 2
    raise KeyError(kind)


def pattern_scene(kind, n, salt=0):
    """-> (xyzw [n,4], desc [n,32], expected indices): one inside and one outside point of PLANTED laid out by the pattern"""
    keep = pattern(kind, n)
    rows = np.arange(n)
    xyz = np.where(keep[:, None], INSIDE_POINT, OUTSIDE_POINT).astype(F)
    xyzw = np.concatenate([xyz, signature_w(rows)[:, None]], axis=1).astype(F)
    return xyzw, signature_desc(rows, salt), np.flatnonzero(keep).astype(np.int32)


def random_cloud(rng, n, name="planted"):
    """points in a box around the frustum, roughly half of them kept (as tools/bench_clip.py)"""
    p = PROJECTORS[name]
    z = rng.uniform(0.6 * p["range_min"], 1.25 * p["range_max"], n)
    u = rng.uniform(-0.1, 1.1, n) * p["canvas_cols"]
    v = rng.uniform(-0.1, 1.1, n) * p["canvas_rows"]
    xyz = np.stack([(u - p["cx"]) * z / p["fx"], (v - p["cy"]) * z / p["fy"], z], axis=-1)
    return np.concatenate([xyz, rng.uniform(1.0, 4.0, (n, 1))], axis=1).astype(F)


def general_pose(rng, scale=1.0):
    R = hp.rot("y", rng.uniform(-0.3, 0.3) * scale) @ hp.rot("x", rng.uniform(-0.2, 0.2) * scale) @ hp.rot("z", rng.uniform(-0.2, 0.2) * scale)
    R[:3, 3] = rng.uniform(-0.4, 0.4, 3) * scale
    return R.astype(F)


def ages(rng, n):
    """every value of AGES, irregularly, and each of them in the first rows"""
    a = AGES[rng.integers(0, len(AGES), n)]
    a[: min(n, len(AGES))] = AGES[: min(n, len(AGES))]
    return a.astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------ batches
def blank(key, B, stride, proj, S):
    xyzw = np.empty((B, stride, 4), F)
    xyzw[:, :, :3] = INSIDE_POINT if proj == "planted" else np.array([0.5, 0.25, 1.0], F)  # rows past n_scene would be kept
    xyzw[:, :, 3] = -1.0
    return dict(key=key, proj=proj, S=np.asarray(S, F).reshape(4, 4).copy(), stride=stride, xyzw=xyzw,
                desc=np.full((B, stride, 32), 0xEE, np.uint8), n_scene=np.zeros(B, np.int32),
                R=np.tile(I4, (B, 1, 1)), n_opt=np.zeros((B, stride), np.uint32), names=[""] * B)


def put_scene(batch, b, name, xyzw, desc=None, R=I4, n_scene=None):
    n = len(xyzw)
    batch["xyzw"][b, :n] = xyzw
    batch["desc"][b, :n] = signature_desc(np.arange(n), b) if desc is None else desc
    batch["n_scene"][b] = n if n_scene is None else n_scene
    batch["R"][b] = R
    batch["names"][b] = name


@functools.lru_cache(maxsize=None)
def ragged(B, stride):
    """B scenes of one launch.  The first 127 hold every edge of the row count, the keep patterns, the planted edges and a blind
    pose, so that the count + scatter launch of batch[:127] meets them too; the rest are random clouds of random length."""
    rng = np.random.default_rng(1000 + stride)
    batch = blank("ragged-%d-%d" % (B, stride), B, stride, "planted", I4)
    edges = sorted({0, 1, WAVE - 1, WAVE, WAVE + 1, SUB - 1, SUB, SUB + 1}
                   | {t * TILE + d for t in range(1, stride // TILE + 1) for d in (-1, 0, 1) if t * TILE + d <= stride}
                   | {stride - 1, stride})
    b = 0
    for n in edges:
        put_scene(batch, b, "n=%d" % n, random_cloud(rng, n), R=general_pose(rng, 0.3))
        b += 1
    put_scene(batch, b, "n=stride+5", random_cloud(rng, stride), R=general_pose(rng, 0.3), n_scene=stride + 5)
    put_scene(batch, b + 1, "n=-3", random_cloud(rng, stride), R=general_pose(rng, 0.3), n_scene=-3)
    b += 2
    for kind in PATTERNS:
        xyzw, desc, _ = pattern_scene(kind, stride, b)
        put_scene(batch, b, "pattern:" + kind, xyzw, desc)
        b += 1
    c = edge_cloud("planted")
    put_scene(batch, b, "edges", c["xyzw"], c["desc"])
    put_scene(batch, b + 1, "blind", random_cloud(rng, stride - 7), R=hp.rot("x", np.pi))
    # the last row inside and the rows behind it inside too: only `i < n` keeps them out
    tail = np.concatenate([random_cloud(rng, 1499), np.array([[*INSIDE_POINT, 9.0]], F)])
    put_scene(batch, b + 2, "inside_tail", tail)
    b += 3
    assert b <= 127, b
    while b < B:
        n = int(rng.integers(1, stride + 1))
        put_scene(batch, b, "random", random_cloud(rng, n), R=general_pose(rng, 0.3))
        b += 1
    for s in range(B):
        batch["n_opt"][s] = ages(rng, stride)
    return batch


def head(batch, count):
    """the first `count` scenes of a batch as a batch of its own"""
    out = dict(batch)
    for key in ("xyzw", "desc", "n_scene", "R", "n_opt", "names"):
        out[key] = batch[key][:count]
    return out


def rows_of(batch, b):
    return int(min(max(int(batch["n_scene"][b]), 0), batch["stride"]))


_EXPECTED = {}


def expected(batch, b, with_nopt=False):
    """scene_clip_ref.clip of scene b (the scene clamped to [0, stride] rows), computed once per process"""
    key = (batch["key"], b, with_nopt)
    if key not in _EXPECTED:
        n = rows_of(batch, b)
        _EXPECTED[key] = ref.clip(plain(batch["proj"]), batch["R"][b], batch["S"], batch["xyzw"][b, :n], batch["desc"][b, :n],
                                  batch["n_opt"][b, :n] if with_nopt else None)
    return _EXPECTED[key]


@functools.lru_cache(maxsize=None)
def small(stride):
    """three scenes at one stride for the walk with one and two tiles and for the ages: the tall projector's edges, an irregular
    pattern of kept rows behind dropped ones, a random cloud"""
    rng = np.random.default_rng(77 + stride)
    batch = blank("small-%d" % stride, 3, stride, "tall", I4)
    c = edge_cloud("tall")
    n = min(stride, len(c["xyzw"]))
    put_scene(batch, 0, "edges", c["xyzw"][:n], c["desc"][:n])
    put_scene(batch, 1, "random", random_cloud(rng, stride, "tall"), R=general_pose(rng, 0.2))
    put_scene(batch, 2, "short", random_cloud(rng, max(stride - 300, 1), "tall"))
    for s in range(3):
        batch["n_opt"][s] = ages(rng, stride)
    return batch


@functools.lru_cache(maxsize=None)
def sensor_offsets():
    """name -> (sensor_in_robot, takes the robot-frame branch)"""
    rng = np.random.default_rng(5)
    minus = I4.copy()
    minus[minus == 0] = -0.0
    ulp = I4.copy()
    ulp[0, 0] = np.nextafter(F(1), F(2))
    gen = general_pose(rng, 0.5)
    return {"identity": (I4.copy(), False), "minus_zero": (minus, False), "one_ulp": (ulp, True), "general": (gen, True)}


@functools.lru_cache(maxsize=None)
def sensor_scene():
    """one cloud of 1500 rows under a general pose for the sensor offsets"""
    rng = np.random.default_rng(6)
    xyzw = random_cloud(rng, 1500)
    return xyzw, signature_desc(np.arange(1500), 3), general_pose(rng, 0.3)


def tile_counts(batch):
    return sorted({-(-rows_of(batch, b) // TILE) for b in range(len(batch["n_scene"]))})
