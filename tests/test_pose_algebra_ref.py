"""The pose algebra on the CPU: the cases of tests/pose_algebra_cases.py are what their names promise, and the oracle's float32
restatement of csrc/prs_se3.h (se3_inverse, se3_mul, motion_predict, gn_step) stays within a bound of the float64 reference
(tests/pose_algebra_ref.py) that does NOT grow towards a half turn.  The GPU suite then holds the device to the oracle's bits."""
import collections

import numpy as np
import pytest

import pose_algebra_cases as pa
import pose_algebra_ref as ref
import pose_graph_ref as pg

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


@pytest.fixture
def variant(oracle):
    yield oracle.set_variant
    oracle.set_variant()


# ---- the cases are what they promise ----
def test_pose_cases_take_the_promised_branch():
    count = collections.Counter()
    flips = collections.Counter()
    for c in pa.poses():
        b, fl = pa.branch_f32(c["T"])
        assert b == c["branch"], (c["name"], b)
        assert fl == c["flip"], (c["name"], fl)
        count[(c["family"], b)] += 1
        flips[fl] += 1
        if c["family"] == "tied":
            T = c["T"]
            assert T[0, 0] == T[1, 1] and (c["tied"] == 2 or T[1, 1] == T[2, 2]) and T[0, 0] >= T[2, 2], c["name"]
        if c["drift"]:
            assert c["drift"] / 3 < pa.off_so3(c["T"]) < 3 * c["drift"], (c["name"], pa.off_so3(c["T"]))
        else:
            assert pa.off_so3(c["T"]) < 1e-6, c["name"]
    print("cases per (family, branch):", dict(sorted(count.items())))
    print("q0 < 0:", dict(flips))
    uses = {"axis_x": (0, 1), "axis_y": (0, 2), "axis_z": (0, 3), "axis_random": (0, 1, 2, 3), "tied": (1,),
            "drift_1e-06": (0, 1, 2, 3), "drift_0.001": (0, 1, 2, 3)}
    assert {f for f, _ in count} == set(uses)
    for fam, branches in uses.items():
        assert {b for f, b in count if f == fam} == set(branches), fam
        for b in branches:
            assert count[(fam, b)] >= 20, (fam, b, count[(fam, b)])
    assert flips[True] >= 20 and flips[False] >= 20
    lengths = {round(float(np.linalg.norm(c["T"][:3, 3].astype(np.float64))), 3) for c in pa.poses()}
    assert lengths == {0.0, 1.0, 1000.0}
    # the half turn as exactly as float32 allows: symmetric, so q0 == 0 and nothing flips
    for c in pa.poses():
        if abs(c.get("angle", 0.0)) == pa.PI and not c["drift"]:
            assert np.array_equal(c["T"][:3, :3], c["T"][:3, :3].T), c["name"]


def test_the_oracle_takes_the_same_branch_and_sign(oracle):
    """the selection restated in pose_algebra_cases.branch_f32 is the oracle's: the component the branch computes first (0.5 sqrt(..))
    is the positive one, and w >= 0"""
    for c in pa.poses():
        v = oracle.t2tnq(c["T"])
        n2 = float(np.sum(v[3:].astype(np.float64) ** 2))
        assert n2 <= 1.0 + 1e-6, c["name"]
        if c["branch"] and abs(c["angle"]) != pa.PI:
            i = c["branch"] - 1
            assert (v[3 + i] < 0) == c["flip"] and abs(v[3 + i]) > 0.4, (c["name"], v)  # flipped with q0 when q0 < 0


def test_solver_cases_are_what_they_promise():
    names = [s["name"] for s in pa.systems()]
    assert len(set(names)) == len(names)
    for s in pa.systems():
        H = s["H"].astype(np.float64).reshape(6, 6)
        for form in (ref.DAMPING_DIAG, ref.DAMPING_IDENTITY):
            d = ref.ldlt_pivots(ref.damped(H, s["damping"], form))
            if s["expect"] == "bad_pivot":
                assert len(d) == s["pivot"] + 1 and not d[-1] > 0.0, (s["name"], form, d)
            else:
                assert len(d) == 6 and np.all(d > 0.0), (s["name"], form, d)
        if s["group"] == "spd":
            assert 0.5 * s["cond"] < np.linalg.cond(np.tril(H) + np.tril(H, -1).T) < 2.0 * s["cond"], s["name"]
    assert max(s["cond"] for s in pa.systems() if s["group"] == "spd") == 1e6
    for j in range(6):
        s = pa.system("negative_pivot_%d" % j)
        d = ref.ldlt_pivots(ref.damped(s["H"], 0.0, 0))
        assert np.all(d[:-1] >= 0.9) and np.all(d[:-1] <= 10.1) and abs(d[-1] + 1.0) < 1e-4, d
    assert pa.system("zero_pivot_0")["H"][0] == 0.0 and not pa.system("zero_matrix")["H"].any()
    assert np.isnan(pa.system("nan_lower_triangle")["H"].reshape(6, 6)[3, 1]) and np.isnan(pa.system("nan_rhs")["b"]).sum() == 1
    up = pa.system("nan_upper_triangle")["H"].reshape(6, 6)
    assert np.isnan(up[np.triu_indices(6, 1)]).all() and np.array_equal(_bits(np.tril(up)), _bits(np.tril(pa.system("clean")["H"].reshape(6, 6))))
    den, big, inf = (pa.system("pivot_" + t)["H"][7 * at] for t, at in (("denormal", 5), ("2p127", 2), ("inf", 2)))
    assert 0.0 < den < f32(2.0 ** -126) and big == f32(2.0 ** 127) and np.isposinf(inf)
    one = [pa.system("unit_step_" + t)["b"][3] for t in ("2", "1", "below_1")]
    assert one[0] == -2.0 and one[1] == -1.0 and _bits(-one[2])[()] == _bits(f32(1.0))[()] - 1


# ---- the oracle against float64 ----
def _predict_before_the_fix(oracle, P2, P1):
    """motion_predict as it was: the real part recovered by tnq2t at every angle (composed from the oracle's own functions)"""
    raw = oracle.se3_mul(P1, oracle.se3_mul(oracle.se3_inverse(P2), P1))
    return oracle.tnq2t(oracle.t2tnq(raw))


def _evaluations(oracle):
    """(case, what, positive path, rotation error, translation error, rotation error before the fix or None)"""
    cs = pa.poses()
    out = []
    for n, c in enumerate(cs):
        T = c["T"]
        U = cs[(n + 7) % len(cs)]["T"] if not c["drift"] else pa.STEP_BIG.astype(f32)
        positive = c["branch"] == 0
        w = ref.inverse(T)
        g = oracle.se3_inverse(T)
        out.append((c, "inverse", positive, ref.rotation_error(w, g), ref.translation_error(w, g), None))
        w = ref.product(T, U)
        g = oracle.se3_mul(T, U)
        out.append((c, "product", positive, ref.rotation_error(w, g), ref.translation_error(w, g), None))
        w = ref.product(T, ref.inverse(U))
        g = oracle.se3_mul(T, oracle.se3_inverse(U))  # pose_compose
        out.append((c, "compose", positive, ref.rotation_error(w, g), ref.translation_error(w, g), None))
        for kind in pa.P2_KINDS:
            P2 = pa.previous_pose(T, kind)
            w = ref.motion_predict(P2, T)
            g = oracle.motion_predict(P2, T)
            angle = ref.rotation_error(np.eye(4), w)
            old = _predict_before_the_fix(oracle, P2, T)
            out.append((c, "predict_" + kind, angle < pa.SEAM - 0.01, ref.rotation_error(w, g), ref.translation_error(w, g), ref.rotation_error(w, old)))
    return out


def test_oracle_against_float64(oracle):
    """4 x the error measured where the positive-trace path rebuilds the rotation, over ALL cases: the bound does not grow with the
    angle.  With motion_predict as it was (w recovered from the imaginary part at every angle) the half-turn family fails it:
    before the fix the families on SO(3) measured 4.9e-6 / 5.3e-5 / 1.0e-3 / 1.0e-4 rad at pi - 0.1 / 1e-2 / 1e-3 / 1e-4 (P2 = P1;
    from pi - 1e-3 on the recovered w rounds to 0 and the error is the distance to the half turn), after it 1.8e-7 / 2.5e-7 /
    2.0e-7 / 2.0e-7 (profiles/pose_algebra/README.md)."""
    ev = _evaluations(oracle)
    measured_rot, measured_trans = collections.defaultdict(float), collections.defaultdict(float)
    for c, what, positive, er, et, _ in ev:
        if positive:
            measured_rot[c["drift"]] = max(measured_rot[c["drift"]], er)
            measured_trans[c["drift"]] = max(measured_trans[c["drift"]], et)
    print("measured on the positive-trace path, per drift level: rotation", dict(measured_rot), "translation", dict(measured_trans))
    print("constants: rotation", pa.MEASURED_ROT, "translation", pa.MEASURED_TRANS)
    for delta in pa.HALF_TURN_DELTAS:
        rows = [(er, old) for c, what, _, er, _, old in ev
                if what == "predict_same" and not c["drift"] and abs(abs(c.get("angle", 0.0)) - (pa.PI - delta)) < 1e-12]
        print("half turn, pi - %g, %d cases: before the fix %.2e rad, after %.2e rad" % (delta, len(rows), max(r[1] for r in rows), max(r[0] for r in rows)))
        assert max(r[1] for r in rows) > 2.0 * 4.0 * pa.MEASURED_ROT[0.0] or delta > 0.05  # the defect is real and this bound sees it
    for d in pa.DRIFTS:  # the constants are the measurement (within its noise across libms), not a wish
        assert 0.5 * pa.MEASURED_ROT[d] <= measured_rot[d] <= 1.25 * pa.MEASURED_ROT[d], (d, measured_rot[d])
        assert 0.5 * pa.MEASURED_TRANS[d] <= measured_trans[d] <= 1.25 * pa.MEASURED_TRANS[d], (d, measured_trans[d])
    worst = max(ev, key=lambda e: e[3] / pa.MEASURED_ROT[e[0]["drift"]])
    print("worst rotation: %s %s %.2e" % (worst[0]["name"], worst[1], worst[3]))
    for c, what, _, er, et, _ in ev:
        assert er <= 4.0 * pa.MEASURED_ROT[c["drift"]], (c["name"], what, er)
        assert et <= 4.0 * pa.MEASURED_TRANS[c["drift"]], (c["name"], what, et)


def test_motion_predict_below_the_seam_is_what_it_was(oracle):
    """the positive-trace path is untouched: the same bits as the round trip through the oracle's t2tnq and tnq2t"""
    n = 0
    for c in pa.poses():
        for kind in pa.P2_KINDS:
            P2 = pa.previous_pose(c["T"], kind)
            raw = oracle.se3_mul(c["T"], oracle.se3_mul(oracle.se3_inverse(P2), c["T"]))
            if pa.branch_f32(raw)[0] == 0:
                assert np.array_equal(_bits(oracle.motion_predict(P2, c["T"])), _bits(_predict_before_the_fix(oracle, P2, c["T"]))), (c["name"], kind)
                n += 1
    assert n > 500


def _gn(oracle, s, form, X=None):
    X = pa.X0 if X is None else X
    oracle.set_variant(damping_form=form)
    return oracle.gn_step(oracle.linear_system(s["H"], s["b"]), s["damping"], X)


def test_gn_step_against_float64(oracle, variant):
    mr = mt = 0.0
    rows = []
    for s in pa.systems():
        for form in (ref.DAMPING_DIAG, ref.DAMPING_IDENTITY):
            X, rc = _gn(oracle, s, form)
            Xw, rcw = ref.gn_step(s["H"], s["b"], s["damping"], form, pa.X0)
            assert rc == rcw, (s["name"], form, rc, rcw)
            if s["expect"] == "bad_pivot":
                assert rc == 1 and np.array_equal(_bits(X), _bits(pa.X0)), s["name"]
            elif s["expect"] == "nan_result":
                assert rc == 0 and (form == ref.DAMPING_IDENTITY and s["name"] == "pivot_denormal" or not np.isfinite(X).all()), s["name"]
            else:
                assert rc == 0 and np.isfinite(X).all(), (s["name"], form)
            if s["group"] == "spd":
                er, et = ref.rotation_error(Xw, X), ref.translation_error(Xw, X)
                rows.append((s, er, et))
                if s["cond"] <= 1e3:
                    mr, mt = max(mr, er), max(mt, et)
    print("gn_step, SPD systems of condition <= 1e3: rotation %.2e translation %.2e (constants %.2e %.2e)" % (mr, mt, pa.MEASURED_GN_ROT, pa.MEASURED_GN_TRANS))
    for cond in sorted({s["cond"] for s, _, _ in rows}):
        print("  condition %g: rotation %.2e translation %.2e" % (cond, max(r[1] for r in rows if r[0]["cond"] == cond), max(r[2] for r in rows if r[0]["cond"] == cond)))
    assert 0.5 * pa.MEASURED_GN_ROT <= mr <= 1.25 * pa.MEASURED_GN_ROT and 0.5 * pa.MEASURED_GN_TRANS <= mt <= 1.25 * pa.MEASURED_GN_TRANS
    for s, er, et in rows:
        if s["cond"] <= 1e3:
            assert er <= 10.0 * pa.MEASURED_GN_ROT and et <= 10.0 * pa.MEASURED_GN_TRANS, (s["name"], er, et)


def test_gn_step_edges(oracle, variant):
    for form in (ref.DAMPING_DIAG, ref.DAMPING_IDENTITY):
        clean, rc0 = _gn(oracle, pa.system("clean"), form)
        dirty, rc1 = _gn(oracle, pa.system("nan_upper_triangle"), form)
        assert rc0 == rc1 == 0 and np.array_equal(_bits(clean), _bits(dirty))  # the upper triangle is not read
        # |dq| = 2 and |dq| = 1: the step is a half turn about x (w = 0); just below 1: w = sqrt(1 - n2) is tiny but not 0
        I4 = np.eye(4, dtype=f32)
        half = np.diag([1.0, -1.0, -1.0, 1.0]).astype(f32)
        for tag in ("2", "1"):
            X, rc = _gn(oracle, pa.system("unit_step_" + tag), form, I4)
            assert rc == 0 and np.array_equal(X, half), (tag, X)
        X, rc = _gn(oracle, pa.system("unit_step_below_1"), form, I4)
        assert rc == 0 and X[2, 1] > 0 and X[1, 2] < 0 and abs(X[2, 1]) < 1e-3 and not np.array_equal(X, half)
        # the reciprocal of a pivot of 2^127 is a denormal, that of +inf is 0: the coordinate does not move
        for tag in ("2p127", "inf"):
            X, rc = _gn(oracle, pa.system("pivot_" + tag), form)
            assert rc == 0 and np.isfinite(X).all(), tag


# ---- the pose graphs of the GPU suite ----
def test_graph_cases_take_the_promised_branch_and_match_the_dense_solver():
    import pose_graph_cases as pc
    for c in pa.graphs():
        A = pg.se3_mul(pg.se3_inverse(c["poses"][0]), c["poses"][1])
        E = pg.se3_mul(pg.se3_inverse(c["Z"][0].astype(np.float64)), A)
        b, fl = pa.branch_f64(E)
        assert b == c["branch"] and (c["flip"] is None or fl == c["flip"]), (c["name"], b, fl)
    seen = {c["branch"] for c in pa.graphs()}
    assert seen == {0, 1, 2, 3} and any(c["flip"] for c in pa.graphs())
    # Gauss-Newton, 3 iterations as the GPU suite runs them, damping 0: the restatement against the dense solver, as
    # test_pose_graph_ref.py does (the exact half turn about x has a zero pivot: both report ERR_NOT_POSITIVE)
    for c in pa.graphs():
        a = pg.optimize(c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], None, 0.0, pg.DAMPING_DIAG, 3, 0.0)
        d = pg.optimize_dense(c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], None, 0.0, pg.DAMPING_DIAG, 3, 0.0)
        assert a["status"] == d["status"], c["name"]
        if a["status"] == 0:
            dt, dq = pc.pose_difference(a["X"], d["X"])
            assert dt <= 10 * pc.MEASURED_MAX_DT and dq <= 10 * pc.MEASURED_MAX_DQ, (c["name"], dt, dq)
