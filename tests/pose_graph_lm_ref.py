"""float64 references of the Levenberg-Marquardt pose-graph optimiser (include/proslam_hip.h, prs_pose_graph_optimize_lm_batch).

optimize_lm        the restatement: linearisation and solve are pose_graph_ref's (the kernel's operation order), the round / trial
                   loop, the `scale` chain and the lambda schedule are written here in the order csrc/pose_graph.hip performs them.
optimize_lm_dense  the same loop on pose_graph_ref._linearize_dense / _solve_dense.
Both return dict(X, chi, chi_final, lam, trials, rho, accepted, linearizations, iterations, envelope_blocks, status, trials_total,
rejected_not_positive_definite, stalled); rho and accepted are per round lists over the trials (rho None at a failed pivot).
"""
import numpy as np

import pose_graph_ref as ref

# icl.conf:665-685, tum.conf:174-194
SHIPPED = dict(user_lambda_init=0.0, tau=1e-5, step_high=0.666667, step_low=0.333333, lm_iterations_max=100, variable_damping=1)


def _scale(dx, d, g, lam, variable_damping, fixed):
    """sum over the scalar rows of free nodes, ascending, from +0, of dx_r * ((lambda * D_r) * dx_r + g_r), then + 1e-3"""
    acc = np.float64(0.0)
    for r in range(len(dx)):
        if fixed[r // 6]:
            continue
        D = d[r] if variable_damping else np.float64(1.0)
        acc = acc + dx[r] * ((lam * D) * dx[r] + g[r])
    return acc + np.float64(1e-3)


def _run_lm(poses, fixed, src, dst, Z, omega, lm, max_iterations, epsilon, linearize, solver, caps):
    f32 = lambda v: np.float64(np.float32(v))
    X = np.asarray(poses, np.float64).reshape(-1, 16).copy()
    n = len(X)
    fixed = np.asarray(fixed).astype(bool).reshape(-1)
    src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
    out = dict(X=X, chi=[], chi_final=np.float64(0.0), lam=[], trials=[], rho=[], accepted=[], linearizations=0, iterations=0,
               envelope_blocks=0, status=ref.OK, trials_total=0, rejected_not_positive_definite=0, stalled=0)
    out["status"], out["envelope_blocks"] = ref.check_graph(n, src, dst, *caps)
    if out["status"] != ref.OK:
        return out
    E = len(src)
    Z = np.asarray(Z)
    Z = (Z if Z.dtype == np.float64 else Z.astype(np.float32)).reshape(E, 16)
    Om = ref._omega(omega, E)
    first = ref.first_of(n, src, dst)
    eps, user, tau = f32(epsilon), f32(lm["user_lambda_init"]), f32(lm["tau"])
    hi, lo = f32(lm["step_high"]), f32(lm["step_low"])
    variable = bool(lm["variable_damping"])
    form = ref.DAMPING_DIAG if variable else ref.DAMPING_IDENTITY
    free = ~fixed
    free_rows = np.repeat(free, 6)
    lam, nu = np.float64(0.0), np.float64(2.0)
    if E > 0 and free.any():
        for it in range(max_iterations):
            chi, H, b = linearize(X, fixed, src, dst, Z, Om, True)
            out["chi"].append(chi)
            if eps > 0.0 and it > 0 and out["chi"][it - 1] - chi < eps * out["chi"][it - 1]:
                break
            d = np.diag(H).copy()
            if it == 0:
                nu = np.float64(2.0)
                if user > 0.0:
                    lam = user
                else:
                    hmax = d[free_rows].max()
                    if not (hmax > 0.0 and np.isfinite(d[free_rows]).all()):
                        out["status"] = ref.ERR_NOT_POSITIVE
                        break
                    lam = tau * hmax
            g, X0 = -b, X.copy()
            accepted, pivot_failed, t, lam_used = False, False, 0, lam
            rhos, decisions = [], []
            for t in range(1, int(lm["lm_iterations_max"]) + 1):
                lam_used = lam
                # (the kernel linearises again at X0 for t > 1: the same bits, so H and b are reused here)
                dx = solver(H.copy(), b.copy(), first, fixed, lam, form)
                rho, chi_t = None, None
                if dx is None:
                    pivot_failed = True
                    out["rejected_not_positive_definite"] += 1
                else:
                    pivot_failed = False
                    X[free] = ref.se3_mul(X0[free], ref.tnq2t(dx.reshape(n, 6)[free]))
                    chi_t = linearize(X, fixed, src, dst, Z, Om, False)[0]
                    with np.errstate(all="ignore"):
                        rho = (chi - chi_t) / _scale(dx, d, g, lam, variable, fixed)
                    accepted = bool(rho > 0.0 and np.isfinite(chi_t))
                rhos.append(rho)
                decisions.append(accepted)
                if accepted:
                    u = 2.0 * rho - 1.0
                    alpha = 1.0 - u * u * u
                    lam = lam * max(lo, min(alpha, hi))
                    nu = np.float64(2.0)
                    break
                X[:] = X0
                with np.errstate(over="ignore"):
                    lam = lam * nu
                    nu = 2.0 * nu
                if not np.isfinite(lam):
                    break
            out["lam"].append(lam_used)
            out["trials"].append(t)
            out["rho"].append(rhos)
            out["accepted"].append(decisions)
            out["trials_total"] += t
            if not accepted:
                if pivot_failed:
                    out["status"] = ref.ERR_NOT_POSITIVE
                else:
                    out["stalled"] = 1
                break
            out["iterations"] = it + 1
    out["linearizations"] = len(out["chi"])
    out["chi_final"] = linearize(X, fixed, src, dst, Z, Om, False)[0] if E > 0 else np.float64(0.0)
    return out


def _lm(overrides):
    lm = dict(SHIPPED)
    lm.update(overrides or {})
    return lm


def optimize_lm(poses, fixed, src, dst, Z, omega=None, lm=None, max_iterations=10, epsilon=0.0, node_stride=None, edge_stride=None,
                capacity_blocks=None):
    """the LM kernel restated; lm: overrides of SHIPPED"""
    return _run_lm(poses, fixed, src, dst, Z, omega, _lm(lm), max_iterations, epsilon, ref._linearize, ref._solve_envelope,
                   (node_stride, edge_stride, capacity_blocks))


def optimize_lm_dense(poses, fixed, src, dst, Z, omega=None, lm=None, max_iterations=10, epsilon=0.0):
    return _run_lm(poses, fixed, src, dst, Z, omega, _lm(lm), max_iterations, epsilon, ref._linearize_dense, ref._solve_dense,
                   (None, None, None))
