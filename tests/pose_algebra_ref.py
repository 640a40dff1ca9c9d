"""float64 references of the pose algebra of csrc/prs_se3.h, in matrix form: nothing here follows the header's operation order.

inverse / product   numpy.linalg.inv and @.
motion_predict      P1 inv(P2) P1, the rotation block projected onto SO(3) by SVD (the polar factor).
gn_step             numpy.linalg.solve on the damped system (the lower triangle mirrored), then X T(dx) with q = (sqrt(1 - |dq|^2), dq)
                    as the header defines the perturbation; the return code from the pivots of a float64 LDL^T.
rotation_error / translation_error   the two figures the oracle tests bound.
"""
import numpy as np

DAMPING_DIAG, DAMPING_IDENTITY = 0, 1


def _m(T):
    return np.asarray(T, np.float64).reshape(4, 4)


def inverse(T):
    return np.linalg.inv(_m(T))


def product(A, B):
    return _m(A) @ _m(B)


def project_so3(R):
    """the rotation nearest to R in the Frobenius norm (polar factor), determinant + 1"""
    U, _, Vt = np.linalg.svd(np.asarray(R, np.float64))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    return U @ D @ Vt


def motion_predict(P2, P1):
    out = _m(P1) @ np.linalg.inv(_m(P2)) @ _m(P1)
    out[:3, :3] = project_so3(out[:3, :3])
    out[3] = (0.0, 0.0, 0.0, 1.0)
    return out


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def perturbation(dx):
    """[dt; dq] -> isometry: q = (sqrt(1 - |dq|^2), dq); |dq| >= 1: dq normalised, w = 0 (a half turn)"""
    dx = np.asarray(dx, np.float64)
    v = dx[3:].copy()
    n2 = float(v @ v)
    if n2 < 1.0:
        w = np.sqrt(1.0 - n2)
    else:
        v, w = v / np.sqrt(n2), 0.0
    K = skew(v)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + 2.0 * w * K + 2.0 * (K @ K)
    T[:3, 3] = dx[:3]
    return T


def damped(H, damping, form):
    """the system the solver sees: the LOWER triangle of H mirrored, damping on the diagonal in either form"""
    H = np.asarray(H, np.float64).reshape(6, 6)
    A = np.tril(H) + np.tril(H, -1).T
    d = np.diag(A).copy()
    with np.errstate(invalid="ignore"):
        A[np.diag_indices(6)] = d + damping if form == DAMPING_IDENTITY else d + damping * d
    return A


def ldlt_pivots(A):
    """pivots d_j of A = L D L^T without pivoting, float64; stops behind the first one that is not positive (NaN included).
    U_ij = L_ij d_j is kept beside L_ij so that an infinite pivot (L = 0) does not turn into 0 * inf"""
    A = np.asarray(A, np.float64).reshape(6, 6)
    L, U, d = np.eye(6), np.zeros((6, 6)), []
    with np.errstate(all="ignore"):
        for j in range(6):
            dj = A[j, j] - sum(L[j, k] * U[j, k] for k in range(j))
            d.append(dj)
            if not dj > 0.0:
                break
            for i in range(j + 1, 6):
                U[i, j] = A[i, j] - sum(L[i, k] * U[j, k] for k in range(j))
                L[i, j] = U[i, j] / dj
    return np.array(d)


def gn_step(H, b, damping, form, X):
    """-> (X after, return code): 1 and X as it was when a pivot is not positive"""
    A = damped(H, damping, form)
    d = ldlt_pivots(A)
    if len(d) < 6 or not d[-1] > 0.0:
        return _m(X).copy(), 1
    with np.errstate(all="ignore"):
        dx = np.linalg.solve(A, -np.asarray(b, np.float64).reshape(6))
        return _m(X) @ perturbation(dx), 0


def rotation_error(T_ref, T):
    """the angle of R_ref^T R, radians (atan2 of the antisymmetric part and the trace: accurate at 1e-8 and at pi alike)"""
    A = _m(T_ref)[:3, :3].T @ _m(T)[:3, :3]
    s = 0.5 * np.linalg.norm([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]])
    return float(np.arctan2(s, 0.5 * (np.trace(A) - 1.0)))


def translation_error(T_ref, T):
    """|t - t_ref| relative to max(1, |t_ref|)"""
    tr, t = _m(T_ref)[:3, 3], _m(T)[:3, 3]
    return float(np.linalg.norm(t - tr) / max(1.0, np.linalg.norm(tr)))
