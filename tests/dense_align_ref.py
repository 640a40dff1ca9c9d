"""The dense aligner's rule (include/proslam_hip_dense_align.h, "Dense align") restated in numpy: the samples of a live image, their
association with the model view, the error, the gates, the weight, the 29 terms, the reduction in its fixed shape, the camera-frame
system, its rotation, the step and the loop.  Explicit float32 operations in the order the header writes them, vectorised over the
samples; `reduce_loop` restates the reduction a second time as plain loops.  The step is the checker's gn_step (oracle/, bit for
bit the device's prs::gn_step), as in tests/point_align_ref.py.  BUILD-DEFINED: the reference has no dense tracker; this file is the
specification the kernels are compared with, byte for byte.  `linearize_f64` is the independent check: H and b from a float64
finite-difference Jacobian of the residual under X exp(dx).  Test infrastructure only."""
import numpy as np

F = np.float32
PRS_ERR_RANGE = -4
CLAMP, SATURATED = 0, 1
UNMATCHED, INLIER, OUTLIER, REJECTED, INVALID = 0, 1, 2, 3, 4
P = 4                                   # PRS_DENSE_ALIGN_SAMPLES_PER_THREAD
THREADS, WAVE = 256, 64
SUMS = 29
UPPER = [(i, j) for i in range(6) for j in range(i, 6)]
RESULT_FIELDS = ("H", "b", "chi_inliers", "chi_total", "num_inliers", "num_outliers", "num_rejected", "num_invalid", "num_unmatched",
                 "num_samples", "status", "iterations", "steps_taken", "warnings")


def params(camera, depth_type="u16", scale=1.0, range_min=0.1, range_max=10.0, max_distance=0.2, min_normal_cos=0.8,
           robustifier=SATURATED, chi_threshold=0.01, damping=0.0, max_iterations=10, min_num_inliers=100, linearize_only=0):
    return dict(depth_type=depth_type, scale=F(scale), fx=F(camera["fx"]), fy=F(camera["fy"]), cx=F(camera["cx"]), cy=F(camera["cy"]),
                range_min=F(range_min), range_max=F(range_max), max_distance=F(max_distance), min_normal_cos=F(min_normal_cos),
                robustifier=int(robustifier), chi_threshold=F(chi_threshold), damping=F(damping), max_iterations=int(max_iterations),
                min_num_inliers=int(min_num_inliers), linearize_only=int(linearize_only))


def shape_of(rows, cols, step):
    """(rows_s, cols_s, N, chunks)"""
    rows_s, cols_s = (rows + step - 1) // step, (cols + step - 1) // step
    n = rows_s * cols_s
    return rows_s, cols_s, n, (n + THREADS * P - 1) // (THREADS * P)


def depth_point(u, v, d, p):
    return [(u.astype(F) - p["cx"]) / p["fx"] * d, (v.astype(F) - p["cy"]) / p["fy"] * d, d]


def rotate3(X, a):
    return [(X[i, 0] * a[0] + X[i, 1] * a[1]) + X[i, 2] * a[2] for i in range(3)]


def terms(p, X, model_depth, model_normal, live_depth, live_normal, step):
    """every sample of one pair at X [4, 4] float32 -> (cls [N] uint8, T [29, N] float32 terms, M [29, N] bool: which terms are added).
    The images may be read-only views of any strides: only the samples and the model pixels they meet are touched"""
    rows, cols = live_depth.shape
    v, u = np.meshgrid(np.arange(0, rows, step), np.arange(0, cols, step), indexing="ij")
    v, u = v.reshape(-1), u.reshape(-1)
    n = v.size
    with np.errstate(all="ignore"):
        raw = np.asarray(live_depth[::step, ::step]).reshape(-1).astype(F)
        d = p["scale"] * raw
        go = (raw > 0) & (d >= p["range_min"]) & (d <= p["range_max"])
        pt = depth_point(u, v, d, p)
        y = rotate3(X, pt)
        m = [y[i] + X[i, 3] for i in range(3)]
        go &= m[2] > 0
        uf = np.floor((m[0] / m[2] * p["fx"] + p["cx"]) + F(0.5))
        vf = np.floor((m[1] / m[2] * p["fy"] + p["cy"]) + F(0.5))
        assert uf.dtype == F and vf.dtype == F
        go &= (uf >= 0) & (uf < F(cols)) & (vf >= 0) & (vf < F(rows))
        um, vm = np.where(go, uf, F(0)).astype(np.int64), np.where(go, vf, F(0)).astype(np.int64)
        go &= (um < cols) & (vm < rows)
        um, vm = np.where(go, um, 0), np.where(go, vm, 0)
        dm = np.asarray(model_depth[vm, um], F)
        go &= dm > 0
        nr = np.asarray(model_normal[vm, um], F)
        go &= nr[:, 3] > 0
        nn = [nr[:, 0], nr[:, 1], nr[:, 2]]
        f = depth_point(um, vm, dm, p)
        e = [m[i] - f[i] for i in range(3)]
        dist2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        r = (nn[0] * e[0] + nn[1] * e[1]) + nn[2] * e[2]
        chi = r * r
        invalid = go & ~(np.isfinite(dist2) & np.isfinite(chi))
        go &= ~invalid
        passed = dist2 <= p["max_distance"] * p["max_distance"]
        if live_normal is not None:
            ln = np.asarray(live_normal[::step, ::step], F).reshape(-1, 4)
            k = rotate3(X, [ln[:, 0], ln[:, 1], ln[:, 2]])
            passed &= (ln[:, 3] > 0) & ((k[0] * nn[0] + k[1] * nn[1]) + k[2] * nn[2] >= p["min_normal_cos"])
        rejected = go & ~passed
        go &= passed
        inlier = go & (chi <= p["chi_threshold"])
        outlier = go & ~inlier
        weighted = inlier | (outlier & (p["robustifier"] == SATURATED))
        w = np.where(inlier, F(1), F(1) / chi).astype(F)
        g = nn + [y[1] * nn[2] - y[2] * nn[1], y[2] * nn[0] - y[0] * nn[2], y[0] * nn[1] - y[1] * nn[0]]
        T = np.zeros((SUMS, n), F)
        M = np.zeros((SUMS, n), bool)
        for k_, (i, j) in enumerate(UPPER):
            T[k_] = w * (g[i] * g[j])
        for i in range(6):
            T[21 + i] = w * (g[i] * r)
        M[:27] = weighted
        T[27], M[27] = chi, inlier
        T[28], M[28] = np.where(inlier, chi, p["chi_threshold"]), go
    cls = np.zeros(n, np.uint8)
    cls[inlier], cls[outlier], cls[rejected], cls[invalid] = INLIER, OUTLIER, REJECTED, INVALID
    return cls, T, M


def butterfly(s):
    """[..., 64] -> the total every lane ends with, taken from lane 0"""
    lane = np.arange(WAVE)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ m]
    return s[..., 0]


def reduce(T, M):
    """the reduction in its fixed shape, vectorised: T, M [29, N] -> the 29 sums"""
    k, n = T.shape
    chunk = THREADS * P
    chunks = (n + chunk - 1) // chunk
    with np.errstate(all="ignore"):
        Tp, Mp = np.zeros((k, chunks * chunk), F), np.zeros((k, chunks * chunk), bool)
        Tp[:, :n], Mp[:, :n] = T, M
        Tp, Mp = Tp.reshape(k, chunks, P, THREADS), Mp.reshape(k, chunks, P, THREADS)
        s = np.zeros((k, chunks, THREADS), F)
        for j in range(P):
            s = np.where(Mp[:, :, j], s + Tp[:, :, j], s)
        W = butterfly(s.reshape(k, chunks, THREADS // WAVE, WAVE))
        total = ((W[..., 0] + W[..., 1]) + W[..., 2]) + W[..., 3]          # [k, chunks]
        J = (chunks + WAVE - 1) // WAVE
        Cp, Cm = np.zeros((k, J * WAVE), F), np.zeros((k, J * WAVE), bool)
        Cp[:, :chunks], Cm[:, :chunks] = total, True
        Cp, Cm = Cp.reshape(k, J, WAVE), Cm.reshape(k, J, WAVE)
        s = np.zeros((k, WAVE), F)
        for j in range(J):
            s = np.where(Cm[:, j], s + Cp[:, j], s)
        out = butterfly(s)
    assert out.dtype == F
    return out


def reduce_loop(T, M):
    """the same reduction as plain loops over threads, lanes and chunks, one float32 addition at a time"""
    k, n = T.shape
    chunk = THREADS * P
    chunks = (n + chunk - 1) // chunk
    lanes = list(range(WAVE))
    out = np.zeros(k, F)
    with np.errstate(all="ignore"):
        for i in range(k):
            totals = []
            for c in range(chunks):
                thread = [F(0)] * THREADS
                for t in range(THREADS):
                    for j in range(P):
                        q = c * chunk + j * THREADS + t
                        if q < n and M[i, q]:
                            thread[t] = F(thread[t] + T[i, q])
                waves = []
                for w in range(THREADS // WAVE):
                    val = thread[w * WAVE:(w + 1) * WAVE]
                    for m in (32, 16, 8, 4, 2, 1):
                        val = [F(val[l] + val[l ^ m]) for l in lanes]
                    waves.append(val[0])
                totals.append(F(F(F(waves[0] + waves[1]) + waves[2]) + waves[3]))
            val = [F(0)] * WAVE
            for c in range(chunks):
                val[c % WAVE] = F(val[c % WAVE] + totals[c])
            for m in (32, 16, 8, 4, 2, 1):
                val = [F(val[l] + val[l ^ m]) for l in lanes]
            out[i] = val[0]
    return out


def assemble(X, s):
    """the camera-frame system from the sums, rotated: Rt^T Hc Rt, Rt^T bc (the lower triangle mirrored)"""
    Hc, bc = np.zeros((6, 6), F), np.zeros(6, F)
    scale = [F(1), F(1), F(1), F(2), F(2), F(2)]
    for k, (i, j) in enumerate(UPPER):
        Hc[i, j] = Hc[j, i] = (scale[i] * scale[j]) * s[k]
    for i in range(6):
        bc[i] = scale[i] * s[21 + i]
    R = np.asarray(X, F).reshape(4, 4)
    Hn, b = np.zeros((6, 6), F), np.zeros(6, F)
    with np.errstate(all="ignore"):
        for r in range(6):
            blk, i = divmod(r, 3)
            Ri0, Ri1, Ri2 = R[0, i], R[1, i], R[2, i]
            Y = Hc[3 * blk:3 * blk + 3]
            for cb in range(2):
                v = [(Ri0 * Y[0, 3 * cb + c] + Ri1 * Y[1, 3 * cb + c]) + Ri2 * Y[2, 3 * cb + c] for c in range(3)]
                for j in range(3):
                    Hn[r, 3 * cb + j] = (v[0] * R[0, j] + v[1] * R[1, j]) + v[2] * R[2, j]
            b[r] = (Ri0 * bc[3 * blk] + Ri1 * bc[3 * blk + 1]) + Ri2 * bc[3 * blk + 2]
    H = np.zeros((6, 6), F)
    for r in range(6):
        for c in range(r + 1):
            H[r, c] = H[c, r] = Hn[r, c]
    return H, b


def linearize(p, X, model_depth, model_normal, live_depth, live_normal, step, reducer=reduce):
    """one linearisation at X -> dict(H, b, chi_inliers, chi_total, the five counts, num_samples, cls [N], sums [29])"""
    X = np.asarray(X, F).reshape(4, 4)
    cls, T, M = terms(p, X, model_depth, model_normal, live_depth, live_normal, step)
    s = reducer(T, M)
    H, b = assemble(X, s)
    count = lambda c: int((cls == c).sum())  # noqa: E731
    return dict(H=H, b=b, chi_inliers=F(s[27]), chi_total=F(s[28]), num_inliers=count(INLIER), num_outliers=count(OUTLIER),
                num_rejected=count(REJECTED), num_invalid=count(INVALID), num_unmatched=count(UNMATCHED), num_samples=int(cls.size),
                cls=cls, sums=s)


def gn_step(H, b, damping, X):
    """-> (X after, whether the step was taken): the checker's gn_step"""
    from oracle import binding as ob
    Xn, rc = ob.gn_step(ob.linear_system(H, b), float(damping), X)
    return (Xn, True) if rc == 0 else (np.asarray(X, F).reshape(4, 4).copy(), False)


def align(p, X0, model_depth, model_normal, live_depth, live_normal=None, step=1):
    """the whole call for one pair -> (X [4, 4] float32, result dict with the fields of prs_dense_align_result, mask [N] uint8)"""
    X = np.array(X0, F).reshape(4, 4)
    rows, cols = live_depth.shape
    n = shape_of(rows, cols, step)[2]
    res = dict(H=np.zeros((6, 6), F), b=np.zeros(6, F), chi_inliers=F(0), chi_total=F(0), num_inliers=0, num_outliers=0, num_rejected=0,
               num_invalid=0, num_unmatched=0, num_samples=n, status=0, iterations=0, steps_taken=0, warnings=0)
    mask = np.zeros(n, np.uint8)
    if not np.isfinite(X[:3]).all():
        res["warnings"] = PRS_ERR_RANGE
        return X, res, mask
    iterations = 1 if p["linearize_only"] else p["max_iterations"]
    for _ in range(iterations):
        lin = linearize(p, X, model_depth, model_normal, live_depth, live_normal, step)
        for k in RESULT_FIELDS[:10]:
            res[k] = lin[k]
        mask = lin["cls"]
        res["status"] = int(lin["num_inliers"] >= p["min_num_inliers"])
        res["iterations"] += 1
        if res["status"] and not p["linearize_only"]:
            X, taken = gn_step(lin["H"], lin["b"], p["damping"], X)
            res["steps_taken"] += int(taken)
    return X, res, mask


def align_schedule(p, X0, model_depth, model_normal, live_depth, live_normal, schedule):
    """calls with (step, max_iterations) of the schedule on the same X -> (X, the last call's result and mask)"""
    X, res, mask = np.array(X0, F).reshape(4, 4), None, None
    for step, iterations in schedule:
        X, res, mask = align(dict(p, max_iterations=int(iterations)), X, model_depth, model_normal, live_depth, live_normal, step)
    return X, res, mask


# ------------------------------------------------------------------------------------------------------------ float64
def perturbation(dx):
    """[dt; dq] -> isometry, q = (sqrt(1 - |dq|^2), dq)"""
    v = np.asarray(dx[3:], np.float64)
    w = np.sqrt(1.0 - float(v @ v))
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + 2.0 * w * K + 2.0 * (K @ K)
    D[:3, 3] = dx[:3]
    return D


def linearize_f64(p, X, model_depth, model_normal, live_depth, step, cls, h=1e-6):
    """H = sum w J^T J and b = sum w J^T r in float64 over the samples the float32 rule weighted (cls: its classes), with the
    association (the model pixel, its point f and normal n) held as the rule found it at X and J the central finite difference of
    r(dx) = n . (X exp(dx) p - f) -> (H, b)"""
    X = np.asarray(X, np.float64).reshape(4, 4)
    rows, cols = live_depth.shape
    q = {k: float(p[k]) for k in ("fx", "fy", "cx", "cy", "scale", "chi_threshold")}
    v, u = np.meshgrid(np.arange(0, rows, step), np.arange(0, cols, step), indexing="ij")
    v, u = v.reshape(-1), u.reshape(-1)
    keep = (cls == INLIER) | ((cls == OUTLIER) & (p["robustifier"] == SATURATED))
    v, u, c = v[keep], u[keep], cls[keep]
    d = q["scale"] * np.asarray(live_depth, np.float64)[v, u]
    pt = np.stack([(u - q["cx"]) / q["fx"] * d, (v - q["cy"]) / q["fy"] * d, d, np.ones_like(d)])          # [4, n]
    m = X @ pt
    um = np.floor((m[0] / m[2] * q["fx"] + q["cx"]) + 0.5).astype(np.int64)
    vm = np.floor((m[1] / m[2] * q["fy"] + q["cy"]) + 0.5).astype(np.int64)
    dm = np.asarray(model_depth, np.float64)[vm, um]
    f = np.stack([(um - q["cx"]) / q["fx"] * dm, (vm - q["cy"]) / q["fy"] * dm, dm])
    nn = np.asarray(model_normal, np.float64)[vm, um, :3].T

    def residual(dx):
        return ((((X @ perturbation(dx)) @ pt)[:3] - f) * nn).sum(0)

    r = residual(np.zeros(6))
    J = np.stack([(residual(np.eye(6)[i] * h) - residual(-np.eye(6)[i] * h)) / (2.0 * h) for i in range(6)], 1)   # [n, 6]
    w = np.where(c == INLIER, 1.0, 1.0 / (r * r))
    return (J * w[:, None]).T @ J, (J * w[:, None]).T @ r


def pose_error(X, truth):
    """(metres, radians) between two isometries"""
    D = np.linalg.inv(np.asarray(truth, np.float64).reshape(4, 4)) @ np.asarray(X, np.float64).reshape(4, 4)
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.linalg.norm(D[:3, 3])), float(np.arctan2(s, 0.5 * (np.trace(D[:3, :3]) - 1.0)))
