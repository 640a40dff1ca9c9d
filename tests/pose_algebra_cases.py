"""Inputs of the pose-algebra tests (csrc/prs_se3.h: se3_inverse, se3_mul, t2tnq, tnq2t, motion_predict, ldlt_solve6, gn_step),
shared by the CPU suite (tests/test_pose_algebra_ref.py: every case is what its name promises, the oracle against float64) and the
GPU suite (tests/test_pose_algebra_gpu.py: the device against the oracle bit for bit).  numpy only, seeded, built once per process
and never modified by a test.

A pose case is a dict(name, family, drift, T [4, 4] float32, branch, flip): `branch` is the branch of t2tnq the name promises
(0 = positive trace, 1 / 2 / 3 = largest diagonal m00 / m11 / m22), `flip` whether its q0 comes out negative so that the sign flip
runs.  branch_f32() restates t2tnq's SELECTION (not its arithmetic) in float32; the CPU suite checks promise against restatement.
A solver case is a dict(name, group, H [36], b [6] float32, damping, expect): expect is "ok", "bad_pivot" or "nan_result".
"""
import functools

import numpy as np

f32 = np.float32
PI = float(np.pi)
SEAM = 2.0 * PI / 3.0  # trace = 1 + 2 cos(angle) changes sign here
# |angle| of every axis family; pi itself is built as 2 a a^T - I ("as exactly as float32 allows": symmetric, q0 == 0)
ANGLES = (0.0, 1e-4, 1.0, SEAM - 1e-3, SEAM + 1e-3, 2.5, PI - 0.1, PI - 1e-2, PI - 1e-3, PI - 1e-4, PI)
HALF_TURN_DELTAS = (0.1, 1e-2, 1e-3, 1e-4)
DRIFT_ANGLES = (0.5, 1.5, 2.5, PI - 0.1, PI - 1e-2)
TRANSLATIONS = (0.0, 1.0, 1e3)  # metres
DRIFTS = (0.0, 1e-6, 1e-3)

# Largest error of the CPU oracle against the float64 reference (tests/pose_algebra_ref.py) over the evaluations whose rotation is
# rebuilt on the positive-trace path, where motion_predict is what it always was: measured on the CPU by
# tests/test_pose_algebra_ref.py::test_oracle_against_float64 (it prints them); the test asserts 4 x these over ALL cases.  One pair
# per drift level: a rotation block off SO(3) by d is read differently by se3_inverse (the transpose), by the quaternion (diagonal and
# antisymmetric part) and by the reference (the true inverse, the polar factor), and those readings differ at FIRST order in d --
# rotate about z and shear x against z: the antisymmetric part of R S is not zero -- so a drifted family cannot share the exact
# family's bound; within a level the bound must not depend on the angle, and that is what the test asserts.
MEASURED_ROT = {0.0: 4.6e-7, 1e-6: 2.5e-6, 1e-3: 2.8e-3}   # radians, angle of R_ref^T R
# |t - t_ref| / max(1, |t_ref|); the exact families' figure is the cancellation of two translations of 1e3 m in P1 P2^-1 P1
MEASURED_TRANS = {0.0: 5.0e-6, 1e-6: 1.9e-6, 1e-3: 1.9e-3}
# the same for gn_step on the SPD systems of condition <= 1e3 (asserted at 10 x)
MEASURED_GN_ROT = 3.1e-6
MEASURED_GN_TRANS = 3.6e-7


def rotation(axis, angle):
    """Rodrigues in float64; |angle| == pi: 2 a a^T - I exactly symmetric"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    if abs(angle) == PI:
        return 2.0 * np.outer(a, a) - np.eye(3)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def branch_f32(T):
    """(branch, q0 negative) of t2tnq on a float32 pose: the selection only, in float32"""
    m = np.asarray(T, f32).reshape(4, 4)
    t = f32(f32(m[0, 0] + m[1, 1]) + m[2, 2])
    if t > f32(0.0):
        return 0, False
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    return 1 + i, bool(f32(m[k, j] - m[j, k]) < f32(0.0))  # (times 0.5 / sqrt(..) > 0)


def _dominant_axis(rng, i):
    """a random unit axis whose component i is the largest by a margin (so the largest diagonal is m_ii beyond rounding)"""
    while True:
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        sq = np.sort(a * a)
        if sq[2] - sq[1] > 0.1 and np.min(np.abs(a)) > 0.05:
            j = int(np.argmax(np.abs(a)))
            a[[i, j]] = a[[j, i]]
            return a


def _translation(rng, length):
    d = rng.normal(size=3)
    return length * d / np.linalg.norm(d)


def _case(name, family, drift, T, branch, flip, **kw):
    return dict(name=name, family=family, drift=drift, T=np.asarray(T, np.float64).astype(f32), branch=branch, flip=flip, **kw)


def _promise(axis, angle):
    """branch and flip of a rotation by `angle` about `axis`: m_ii = cos + (1 - cos) a_i^2, q0 of branch i = 2 sin(angle) a_i t"""
    if abs(angle) < SEAM:
        return 0, False
    i = int(np.argmax(np.abs(axis)))
    return 1 + i, bool(abs(angle) != PI and angle * axis[i] < 0)


@functools.lru_cache(maxsize=None)
def poses():
    rng = np.random.default_rng(20261018)
    out = []
    unit = np.eye(3)
    for fam in ("axis_x", "axis_y", "axis_z", "axis_random"):
        for mag in ANGLES:
            for sign in (1, -1):
                for length in TRANSLATIONS:
                    for rep in range(3 if fam == "axis_random" else 1):  # a random axis with its largest component at x, y, z in turn
                        axis = unit[("axis_x", "axis_y", "axis_z").index(fam)] if fam != "axis_random" else _dominant_axis(rng, rep)
                        angle = sign * mag
                        b, fl = _promise(axis, angle)
                        out.append(_case("%s_%+.6f_t%g_%d" % (fam, angle, length, rep), fam, 0.0, pose(rotation(axis, angle), _translation(rng, length)),
                                         b, fl, angle=angle, axis=axis))
    # tied diagonals: m00 == m11 (== m22) bit for bit; the selection keeps the first of them
    for tag, axis in (("110", np.array([1.0, 1.0, 0.0])), ("111", np.array([1.0, 1.0, 1.0]))):
        for mag in (PI,) + tuple(PI - d for d in HALF_TURN_DELTAS):
            for sign in (1, -1):
                for length in TRANSLATIONS:
                    angle = sign * mag
                    out.append(_case("tied_%s_%+.6f_t%g" % (tag, angle, length), "tied", 0.0, pose(rotation(axis, angle), _translation(rng, length)),
                                     1, bool(mag != PI and angle < 0), angle=angle, axis=axis / np.linalg.norm(axis), tied=3 if tag == "111" else 2))
    # rotation blocks off SO(3): R (I + d S), S symmetric of Frobenius norm 1 (the antisymmetric part would be a rotation)
    for d in DRIFTS[1:]:
        fam = "drift_%g" % d
        for mag in DRIFT_ANGLES:
            for sign in (1, -1):
                for length in TRANSLATIONS:
                    for i in range(3):
                        for _ in range(2):
                            axis = _dominant_axis(rng, i)
                            S = rng.normal(size=(3, 3))
                            S = S + S.T
                            S /= np.linalg.norm(S)
                            angle = sign * mag
                            b, fl = _promise(axis, angle)
                            out.append(_case("%s_%+.4f_t%g_%d" % (fam, angle, length, len(out)), fam, d,
                                             pose(rotation(axis, angle) @ (np.eye(3) + d * S), _translation(rng, length)), b, fl, angle=angle, axis=axis))
    return tuple(out)


def off_so3(T):
    R = np.asarray(T, np.float64).reshape(4, 4)[:3, :3]
    return float(np.linalg.norm(R.T @ R - np.eye(3)))


STEP_SMALL = pose(rotation((0.3, -0.5, 0.8), 0.02), (0.05, -0.02, 0.6))
STEP_BIG = pose(rotation((-0.6, 0.7, 0.2), 2.5), (0.4, 0.1, -0.3))
P2_KINDS = ("same", "small_step", "big_step", "identity")


def previous_pose(T, kind):
    """P2 for P1 = T.  same: no motion, so the prediction is T's own round trip through the quaternion (the half-turn family stays at
    its angle); small_step / big_step: P2 = P1 * step; identity: the prediction is P1 * P1"""
    T64 = np.asarray(T, np.float64).reshape(4, 4)
    if kind == "same":
        return np.asarray(T, f32).reshape(4, 4).copy()
    if kind == "identity":
        return np.eye(4, dtype=f32)
    return (T64 @ (STEP_SMALL if kind == "small_step" else STEP_BIG)).astype(f32)


# ---- solver systems ----
def _sys(name, group, H, b, damping, expect, **kw):
    return dict(name=name, group=group, H=np.asarray(H, np.float64).astype(f32).reshape(36), b=np.asarray(b, np.float64).astype(f32).reshape(6),
                damping=damping, expect=expect, **kw)


def _spd(rng, cond):
    """A^T A + I with eigenvalues 1 .. cond, and a right-hand side whose step is a small perturbation"""
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    lam = np.logspace(0.0, np.log10(cond), 6)
    A = np.diag(np.sqrt(lam - 1.0)) @ Q.T
    H = A.T @ A + np.eye(6)
    H = 0.5 * (H + H.T)
    dx = rng.normal(0.0, 0.05, 6)
    return H, -(H @ dx)


@functools.lru_cache(maxsize=None)
def systems():
    rng = np.random.default_rng(20261019)
    out = []
    for cond in (1e1, 1e2, 1e3, 1e4, 1e5, 1e6):
        for k in range(3):
            H, b = _spd(rng, cond)
            out.append(_sys("spd_cond%g_%d" % (cond, k), "spd", H, b, (0.0, 1e-3, 1e-6)[k], "ok", cond=cond))
    for j in range(6):  # H = L D L^T, d_j = -1, the others in [1, 10], |L_ij| <= 1
        L = np.tril(rng.uniform(-1.0, 1.0, (6, 6)), -1) + np.eye(6)
        d = rng.uniform(1.0, 10.0, 6)
        d[j] = -1.0
        out.append(_sys("negative_pivot_%d" % j, "bad_pivot", L @ np.diag(d) @ L.T, rng.normal(size=6), 0.0, "bad_pivot", pivot=j))
    good_H, good_b = _spd(rng, 1e2)
    H = good_H.copy()
    H[0, 0] = 0.0
    out.append(_sys("zero_pivot_0", "bad_pivot", H, good_b, 0.0, "bad_pivot", pivot=0))
    out.append(_sys("zero_matrix", "bad_pivot", np.zeros((6, 6)), good_b, 0.0, "bad_pivot", pivot=0))
    H = good_H.copy()
    H[3, 1] = np.nan
    out.append(_sys("nan_lower_triangle", "bad_pivot", H, good_b, 1e-3, "bad_pivot", pivot=3))
    b = good_b.copy()
    b[2] = np.nan
    out.append(_sys("nan_rhs", "nan", good_H, b, 1e-3, "nan_result"))
    out.append(_sys("clean", "upper", good_H, good_b, 1e-3, "ok"))
    H = good_H.copy()
    H[np.triu_indices(6, 1)] = np.nan
    out.append(_sys("nan_upper_triangle", "upper", H, good_b, 1e-3, "ok"))
    # pivots outside the short form of recip_exact (2^-126 <= |d| < 2^126): the long division must give the host's quotient
    # (the denormal is the LAST pivot: its reciprocal overflows to +inf, and times the zeros below an earlier pivot that would be NaN)
    for tag, value, at, expect in (("denormal", 1e-40, 5, "nan_result"), ("2p127", 2.0 ** 127, 2, "ok"), ("inf", np.inf, 2, "ok")):
        H = np.eye(6)
        H[at, at] = value
        out.append(_sys("pivot_" + tag, "long_reciprocal", H, rng.uniform(0.01, 0.1, 6), 1e-3, expect))
    for tag, v in (("2", 2.0), ("1", 1.0), ("below_1", float(np.nextafter(f32(1.0), f32(0.0))))):
        out.append(_sys("unit_step_" + tag, "unit_step", np.eye(6), (0.0, 0.0, 0.0, -v, 0.0, 0.0), 0.0, "ok", dq=v))
    return tuple(out)


def system(name):
    return next(s for s in systems() if s["name"] == name)


X0 = pose(rotation((0.2, 0.9, -0.4), 0.7), (1.5, -0.3, 4.0)).astype(f32)  # the pose every solver case steps from


# ---- two-node pose graphs whose edge error at the guess takes a chosen branch of t2tnq<double> ----
@functools.lru_cache(maxsize=None)
def graphs():
    """node 0 fixed at a generic pose, one edge 0 -> 1 with a generic measurement Z, node 1's guess = X0 Z E: the edge error at the
    guess is Z^-1 (X0^-1 X1) = E up to rounding"""
    rng = np.random.default_rng(20261020)
    X0g = pose(rotation(rng.normal(size=3), 0.8), rng.normal(0, 2.0, 3))
    Zd = pose(rotation(rng.normal(size=3), 0.4), (1.0, 0.2, -0.1))
    Z = Zd.astype(f32)
    unit = np.eye(3)
    specs = [("x_2.5", unit[0], 2.5, 1), ("y_2.5", unit[1], 2.5, 2), ("z_2.5", unit[2], 2.5, 3), ("y_-2.5", unit[1], -2.5, 2),
             ("x_pi", unit[0], PI, 1), ("z_pi", unit[2], PI, 3), ("x_below_seam", unit[0], SEAM - 1e-3, 0), ("x_above_seam", unit[0], SEAM + 1e-3, 1)]
    out = []
    for name, axis, angle, branch in specs:
        E = pose(rotation(axis, angle), (0.05, -0.02, 0.03))
        X1 = X0g @ Z.astype(np.float64) @ E
        out.append(dict(name="graph_" + name, poses=np.stack([X0g.reshape(16), X1.reshape(16)]), fixed=np.array([1, 0], np.uint8),
                        src=np.array([0], np.int32), dst=np.array([1], np.int32), Z=Z.reshape(1, 16), omega=None, branch=branch,
                        flip=None if abs(angle) == PI else angle < 0))  # (at pi the sign of q0 is rounding)
    return tuple(out)


def branch_f64(T):
    """branch_f32 in double, for the pose graph's edge error"""
    m = np.asarray(T, np.float64).reshape(4, 4)
    if (m[0, 0] + m[1, 1]) + m[2, 2] > 0.0:
        return 0, False
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    return 1 + i, bool(m[k, j] - m[j, k] < 0.0)
