"""float64 references of the pose-graph optimiser (include/proslam_hip.h, prs_pose_graph_optimize_batch).

optimize        the restatement: every operation in the order csrc/pose_graph.hip performs it (separate multiplies and adds, the same
                chains), so that numpy gives the kernel's bits.  Edge quantities are evaluated for all edges at once (elementwise numpy
                operations are the same IEEE operations), sums over edges and the factorisation run in the kernel's sequence.
optimize_dense  the independent check: matrix-form Jacobians, a dense 6n x 6n normal matrix and numpy's LU solve.
"""
import numpy as np

OK, WARN_EMPTY_INPUT, ERR_CAPACITY, ERR_RANGE, ERR_NOT_POSITIVE = 0, 1, -2, -4, -10
DAMPING_DIAG, DAMPING_IDENTITY = 0, 1
MAX_ITERATIONS = 32


# ---- SE(3) pieces of csrc/prs_se3.h in double, vectorised over a leading axis ([..., 16] row-major) ----
def se3_inverse(T):
    T = np.asarray(T, np.float64)
    out = np.zeros_like(T)
    tx, ty, tz = T[..., 3], T[..., 7], T[..., 11]
    for i in range(3):
        r0, r1, r2 = T[..., i], T[..., 4 + i], T[..., 8 + i]
        out[..., 4 * i], out[..., 4 * i + 1], out[..., 4 * i + 2] = r0, r1, r2
        out[..., 4 * i + 3] = -((r0 * tx + r1 * ty) + r2 * tz)
    out[..., 15] = 1.0
    return out


def se3_mul(A, B):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.zeros(np.broadcast(A, B).shape, np.float64)
    for i in range(3):
        for j in range(3):
            out[..., 4 * i + j] = (A[..., 4 * i] * B[..., j] + A[..., 4 * i + 1] * B[..., 4 + j]) + A[..., 4 * i + 2] * B[..., 8 + j]
        out[..., 4 * i + 3] = ((A[..., 4 * i] * B[..., 3] + A[..., 4 * i + 1] * B[..., 7]) + A[..., 4 * i + 2] * B[..., 11]) + A[..., 4 * i + 3]
    out[..., 15] = 1.0
    return out


def t2tnq(T):
    """-> (v6 [..., 6], w [...]): translation, imaginary part and real part of the unit quaternion with w >= 0"""
    T = np.asarray(T, np.float64)
    flat = T.reshape(-1, 16)
    v6, ws = np.zeros((len(flat), 6)), np.zeros(len(flat))
    for n, M in enumerate(flat):
        m00, m01, m02, m10, m11, m12, m20, m21, m22 = M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]
        t = (m00 + m11) + m22
        if t > 0.0:
            t = np.sqrt(t + 1.0)
            q0 = 0.5 * t
            t = 0.5 / t
            q1, q2, q3 = (m21 - m12) * t, (m02 - m20) * t, (m10 - m01) * t
        else:
            i = 0
            if m11 > m00:
                i = 1
            if m22 > (m00 if i == 0 else m11):
                i = 2
            if i == 0:
                t = np.sqrt(((m00 - m11) - m22) + 1.0)
                q1 = 0.5 * t
                t = 0.5 / t
                q0, q2, q3 = (m21 - m12) * t, (m10 + m01) * t, (m20 + m02) * t
            elif i == 1:
                t = np.sqrt(((m11 - m22) - m00) + 1.0)
                q2 = 0.5 * t
                t = 0.5 / t
                q0, q3, q1 = (m02 - m20) * t, (m21 + m12) * t, (m01 + m10) * t
            else:
                t = np.sqrt(((m22 - m00) - m11) + 1.0)
                q3 = 0.5 * t
                t = 0.5 / t
                q0, q1, q2 = (m10 - m01) * t, (m02 + m20) * t, (m12 + m21) * t
        nrm = np.sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3)
        s = 1.0 / nrm
        if q0 < 0.0:
            s = -s
        v6[n] = (M[3], M[7], M[11], q1 * s, q2 * s, q3 * s)
        ws[n] = q0 * s
    return v6.reshape(T.shape[:-1] + (6,)), ws.reshape(T.shape[:-1])


def tnq2t(v6):
    v6 = np.asarray(v6, np.float64)
    x, y, z = v6[..., 3].copy(), v6[..., 4].copy(), v6[..., 5].copy()
    n2 = (x * x + y * y) + z * z
    small = n2 < 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(small, np.sqrt(np.where(small, 1.0 - n2, 0.0)), 0.0)
        s = np.where(small, 1.0, 1.0 / np.sqrt(np.where(small, 1.0, n2)))
    x, y, z = np.where(small, x, x * s), np.where(small, y, y * s), np.where(small, z, z * s)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    T = np.zeros(v6.shape[:-1] + (16,))
    T[..., 0], T[..., 1], T[..., 2], T[..., 3] = 1.0 - (tyy + tzz), txy - twz, txz + twy, v6[..., 0]
    T[..., 4], T[..., 5], T[..., 6], T[..., 7] = txy + twz, 1.0 - (txx + tzz), tyz - twx, v6[..., 1]
    T[..., 8], T[..., 9], T[..., 10], T[..., 11] = txz - twy, tyz + twx, 1.0 - (txx + tyy), v6[..., 2]
    T[..., 15] = 1.0
    return T


def _chain(terms):
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def edge_terms(Xf, Xt, Z):
    """error and Jacobians of edges, [E, 16] each -> e [E, 6], Jf, Jt [E, 6, 6] in the kernel's operation order"""
    Z = np.asarray(Z, np.float64)
    A = se3_mul(se3_inverse(Xf), Xt)
    Em = se3_mul(se3_inverse(Z), A)
    e, w = t2tnq(Em)
    n = len(e)
    v = e[:, 3:]
    a = (A[:, 3], A[:, 7], A[:, 11])
    RZ = lambda r, c: Z[:, 4 * r + c]
    Jt, Jf = np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    for i in range(3):
        for j in range(3):
            Jt[:, i, j] = Em[:, 4 * i + j]
            Jf[:, i, j] = -RZ(j, i)
    Jt[:, 3, 3] = Jt[:, 4, 4] = Jt[:, 5, 5] = w
    Jt[:, 3, 4], Jt[:, 3, 5], Jt[:, 4, 3] = -v[:, 2], v[:, 1], v[:, 2]
    Jt[:, 4, 5], Jt[:, 5, 3], Jt[:, 5, 4] = -v[:, 0], -v[:, 1], v[:, 0]
    for i in range(3):
        Jf[:, i, 3] = 2.0 * (RZ(1, i) * a[2] - RZ(2, i) * a[1])
        Jf[:, i, 4] = 2.0 * (RZ(2, i) * a[0] - RZ(0, i) * a[2])
        Jf[:, i, 5] = 2.0 * (RZ(0, i) * a[1] - RZ(1, i) * a[0])
    M = [[w, v[:, 2], -v[:, 1]], [-v[:, 2], w, v[:, 0]], [v[:, 1], -v[:, 0], w]]
    for i in range(3):
        for j in range(3):
            Jf[:, 3 + i, 3 + j] = -((M[i][0] * RZ(j, 0) + M[i][1] * RZ(j, 1)) + M[i][2] * RZ(j, 2))
    return e, Jf, Jt


def _omega(omega, n_edges):
    if omega is None:
        return np.tile(np.eye(6), (n_edges, 1, 1))
    return np.asarray(omega, np.float32).astype(np.float64).reshape(n_edges, 6, 6)


def first_of(n, src, dst):
    first = np.arange(n)
    for a, b in zip(src, dst):
        lo, hi = min(a, b), max(a, b)
        first[hi] = min(first[hi], lo)
    return first


def check_graph(n, src, dst, node_stride=None, edge_stride=None, capacity_blocks=None):
    """-> (status, envelope_blocks): the per-graph checks of the header's table, in the kernel's order"""
    E = len(src)
    if n < 0 or E < 0:
        return ERR_RANGE, 0
    if (node_stride is not None and n > node_stride) or (edge_stride is not None and E > edge_stride):
        return ERR_CAPACITY, 0
    if n == 0:
        return WARN_EMPTY_INPUT, 0
    for a, b in zip(src, dst):
        if a < 0 or a >= n or b < 0 or b >= n or a == b:
            return ERR_RANGE, 0
    first = first_of(n, src, dst)
    blocks = int(np.sum(np.arange(n) - first + 1))
    if capacity_blocks is not None and blocks > capacity_blocks:
        return ERR_CAPACITY, blocks
    return OK, blocks


def _linearize(X, fixed, src, dst, Z, Om, want_system):
    n = len(X)
    e, Jf, Jt = edge_terms(X[src], X[dst], Z)
    Oe = np.stack([_chain([Om[:, k, l] * e[:, l] for l in range(6)]) for k in range(6)], axis=1)
    chi_e = _chain([e[:, k] * Oe[:, k] for k in range(6)])
    chi = np.float64(0.0)
    for c in chi_e:
        chi = chi + c
    if not want_system:
        return chi, None, None
    OJf = np.stack([np.stack([_chain([Om[:, k, l] * Jf[:, l, b] for l in range(6)]) for b in range(6)], axis=1) for k in range(6)], axis=1)
    OJt = np.stack([np.stack([_chain([Om[:, k, l] * Jt[:, l, b] for l in range(6)]) for b in range(6)], axis=1) for k in range(6)], axis=1)
    jtoj = lambda J, OJ: np.stack([np.stack([_chain([J[:, k, a] * OJ[:, k, b] for k in range(6)]) for b in range(6)], axis=1) for a in range(6)], axis=1)
    jtoe = lambda J: np.stack([_chain([J[:, k, a] * Oe[:, k] for k in range(6)]) for a in range(6)], axis=1)
    Hff, Htt, Htf, bf, bt = jtoj(Jf, OJf), jtoj(Jt, OJt), jtoj(Jt, OJf), jtoe(Jf), jtoe(Jt)
    H, b = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    for k, (f, t) in enumerate(zip(src, dst)):
        sf, st = slice(6 * f, 6 * f + 6), slice(6 * t, 6 * t + 6)
        if not fixed[f]:
            H[sf, sf] = H[sf, sf] + Hff[k]
            b[sf] = b[sf] + bf[k]
        if not fixed[t]:
            H[st, st] = H[st, st] + Htt[k]
            b[st] = b[st] + bt[k]
        if not fixed[f] and not fixed[t]:
            if t > f:
                H[st, sf] = H[st, sf] + Htf[k]
            else:
                H[sf, st] = H[sf, st] + Htf[k].T
    return chi, H, b


def _solve_envelope(H, b, first, fixed, damping, damping_form):
    """scalar LDL^T on the row envelope; H's lower triangle is read.  -> dx or None (pivot <= 0 or not finite)"""
    n = len(first)
    N = 6 * n
    U = H.copy()  # strictly lower: u_rc, diagonal: d_r
    for i in range(n):
        for a in range(6):
            r = 6 * i + a
            if fixed[i]:
                U[r, :] = 0.0
                U[r, r] = 1.0
            elif damping_form == DAMPING_IDENTITY:
                U[r, r] = U[r, r] + damping
            else:
                U[r, r] = U[r, r] + damping * U[r, r]
    c0col = np.repeat(6 * first, 6)
    invd, y = np.zeros(N), -b
    for j in range(n):
        c0, d0 = 6 * first[j], 6 * j
        for m in range(c0, d0):
            l = U[d0:d0 + 6, m] * invd[m]
            mask = c0col[m + 1:d0] <= m
            cols = np.arange(m + 1, d0)[mask]
            if len(cols):
                U[d0:d0 + 6, cols] = U[d0:d0 + 6, cols] - l[:, None] * U[cols, m][None, :]
            um = U[d0:d0 + 6, m].copy()
            for a in range(6):
                U[d0 + a, d0:d0 + a + 1] = U[d0 + a, d0:d0 + a + 1] - l[a] * um[:a + 1]
            y[d0:d0 + 6] = y[d0:d0 + 6] - l * y[m]
        for a in range(6):
            m = d0 + a
            d = U[m, m]
            if not (d > 0.0 and np.isfinite(d)):
                return None
            invd[m] = 1.0 / d
            for a2 in range(a + 1, 6):
                r = d0 + a2
                l = U[r, m] * invd[m]
                for c in range(m + 1, r):
                    U[r, c] = U[r, c] - l * U[c, m]
                U[r, r] = U[r, r] - l * U[r, m]
                y[r] = y[r] - l * y[m]
    z = y * invd
    for r in range(N - 1, -1, -1):
        c0 = c0col[r]
        if r > c0:
            z[c0:r] = z[c0:r] - (U[r, c0:r] * invd[c0:r]) * z[r]
    return z


def _run(poses, fixed, src, dst, Z, omega, damping, damping_form, max_iterations, epsilon, linearize, solver, caps):
    X = np.asarray(poses, np.float64).reshape(-1, 16).copy()
    n = len(X)
    fixed = np.asarray(fixed).astype(bool).reshape(-1)
    src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
    out = dict(X=X, chi=[], chi_final=0.0, iterations=0, envelope_blocks=0, status=OK)
    out["status"], out["envelope_blocks"] = check_graph(n, src, dst, *caps)
    if out["status"] != OK:
        return out
    E = len(src)
    Z = np.asarray(Z)
    Z = (Z if Z.dtype == np.float64 else Z.astype(np.float32)).reshape(E, 16)  # float32 is what the kernel reads (float64: CPU studies)
    Om = _omega(omega, E)
    first = first_of(n, src, dst)
    lam, eps = np.float64(np.float32(damping)), np.float64(np.float32(epsilon))
    if E > 0 and not fixed.all():
        for it in range(max_iterations):
            chi, H, b = linearize(X, fixed, src, dst, Z, Om, True)
            out["chi"].append(chi)
            if eps > 0.0 and it > 0 and out["chi"][it - 1] - chi < eps * out["chi"][it - 1]:
                break
            dx = solver(H, b, first, fixed, lam, damping_form)
            if dx is None:
                out["status"] = ERR_NOT_POSITIVE
                break
            free = ~fixed
            X[free] = se3_mul(X[free], tnq2t(dx.reshape(n, 6)[free]))
            out["iterations"] = it + 1
    out["chi_final"] = linearize(X, fixed, src, dst, Z, Om, False)[0] if E > 0 else np.float64(0.0)
    return out


def optimize(poses, fixed, src, dst, Z, omega=None, damping=0.0, damping_form=DAMPING_DIAG, max_iterations=10, epsilon=0.0,
             node_stride=None, edge_stride=None, capacity_blocks=None):
    """the kernel restated.  poses [n, 16] or [n, 4, 4] float64, Z [E, 16] float32, omega [E, 36] float32 or None ->
    dict(X [n, 16], chi [list], chi_final, iterations, envelope_blocks, status)"""
    return _run(poses, fixed, src, dst, Z, omega, damping, damping_form, max_iterations, epsilon, _linearize, _solve_envelope,
                (node_stride, edge_stride, capacity_blocks))


# ---- the independent implementation ----
def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _quat(R):
    """unit quaternion (w, v) of a rotation matrix, w >= 0 (branch on the largest component)"""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], 0, 0, 0], [R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], 0, 0],
                  [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1], 0],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    vals, vecs = np.linalg.eigh(K)
    q = vecs[:, np.argmax(vals)]  # (x, y, z, w)
    if q[3] < 0:
        q = -q
    return q[3], q[:3]


def dense_edge(Xf, Xt, Z):
    """matrix-form error and Jacobians of one edge (4 x 4 float64 inputs)"""
    A = np.linalg.inv(Xf) @ Xt
    Em = np.linalg.inv(Z) @ A
    w, v = _quat(Em[:3, :3])
    e = np.concatenate([Em[:3, 3], v])
    RZt = Z[:3, :3].T
    Jt, Jf = np.zeros((6, 6)), np.zeros((6, 6))
    Jt[:3, :3], Jt[3:, 3:] = Em[:3, :3], w * np.eye(3) + _skew(v)
    Jf[:3, :3], Jf[:3, 3:], Jf[3:, 3:] = -RZt, 2.0 * RZt @ _skew(A[:3, 3]), -(w * np.eye(3) - _skew(v)) @ RZt
    return e, Jf, Jt


def _solve_dense(H, b, first, fixed, damping, damping_form):
    H = np.tril(H) + np.tril(H, -1).T
    for i in np.nonzero(fixed)[0]:
        s = slice(6 * i, 6 * i + 6)
        H[s, :], H[:, s], b[s] = 0.0, 0.0, 0.0
    D = np.diag(np.diag(H)) if damping_form == DAMPING_DIAG else np.eye(len(H))
    H = H + damping * D
    for i in np.nonzero(fixed)[0]:
        H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = np.eye(6)
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(H, -b)


def _linearize_dense(X, fixed, src, dst, Z, Om, want_system):
    n = len(X)
    H, b, chi = np.zeros((6 * n, 6 * n)), np.zeros(6 * n), 0.0
    for k, (f, t) in enumerate(zip(src, dst)):
        e, Jf, Jt = dense_edge(X[f].reshape(4, 4), X[t].reshape(4, 4), np.asarray(Z[k], np.float64).reshape(4, 4))
        chi += e @ Om[k] @ e
        J = np.zeros((6, 6 * n))
        J[:, 6 * f:6 * f + 6], J[:, 6 * t:6 * t + 6] = Jf, Jt
        if want_system:
            H += J.T @ Om[k] @ J
            b += J.T @ Om[k] @ e
    return chi, H, b


def optimize_dense(poses, fixed, src, dst, Z, omega=None, damping=0.0, damping_form=DAMPING_DIAG, max_iterations=10, epsilon=0.0):
    return _run(poses, fixed, src, dst, Z, omega, damping, damping_form, max_iterations, epsilon, _linearize_dense, _solve_dense,
                (None, None, None))
