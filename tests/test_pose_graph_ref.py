"""The pose-graph optimiser's float64 references (no GPU): Jacobians against central differences, recovery of ground truth from
consistent measurements, the termination rule, and the kernel's restatement against the independent dense implementation."""
import json
import os

import numpy as np
import pytest

import pose_graph_cases as pc
import pose_graph_ref as ref


def _run(f, c, **kw):
    return f(c["poses"], c["fixed"], c["src"], c["dst"], kw.pop("Z", c["Z"]), c["omega"], **kw)


def test_kitti_case_has_the_stated_size():
    k = pc.kitti_case()
    status, blocks = ref.check_graph(len(k["poses"]), k["src"], k["dst"])
    assert status == ref.OK
    assert (len(k["poses"]), len(k["src"]), len(k["src"]) - (len(k["poses"]) - 1), blocks) == (114, 125, 12, 1064)


def test_jacobians_against_central_differences():
    """both Jacobians, restated and matrix form, against float64 central differences (step 1e-6) on random edges, to 1e-7"""
    rng = np.random.default_rng(7)
    h = 1e-6
    for _ in range(16):
        Xf, Xt = pc._rand_pose(rng, 3.0, 0.4), pc._rand_pose(rng, 3.0, 0.4)
        Z = ref.se3_mul(ref.se3_mul(ref.se3_inverse(Xf), Xt), pc._rand_pose(rng, 0.3, 0.2))  # (float64: an exact isometry)
        e, Jf, Jt = ref.edge_terms(Xf[None], Xt[None], Z[None])
        e2, Jf2, Jt2 = ref.dense_edge(Xf.reshape(4, 4), Xt.reshape(4, 4), Z.reshape(4, 4))
        assert np.abs(e[0] - e2).max() < 1e-12 and np.abs(Jf[0] - Jf2).max() < 1e-12 and np.abs(Jt[0] - Jt2).max() < 1e-12

        def error(which, d):
            P = ref.tnq2t(d)
            xf = ref.se3_mul(Xf, P) if which == 0 else Xf
            xt = ref.se3_mul(Xt, P) if which == 1 else Xt
            return ref.edge_terms(xf[None], xt[None], Z[None])[0][0]

        for which, J in ((0, Jf[0]), (1, Jt[0])):
            for a in range(6):
                d = np.zeros(6)
                d[a] = h
                numeric = (error(which, d) - error(which, -d)) / (2 * h)
                assert np.abs(numeric - J[:, a]).max() <= 1e-7, (which, a)


def test_recovery_of_ground_truth_from_consistent_measurements():
    """Z = G_from^-1 G_to exactly (float64, between the SE(3) projections of the stored float32 rows), the guess is the perturbed
    chain, damping 0, criterion on: the optimiser returns to the stored ground truth within 1e-4 m and 1e-6 quaternion units (the
    floor is the stored rows' distance from SE(3): measured 8.5e-12 m and 3.8e-8 after 6 iterations, chi 1.7e3, 31.5, 3.4e-3,
    1.1e-5, 1.3e-15, 2.4e-25).  With the measurements rounded to float32, as the kernel reads them, the same run ends at chi 2.2e-12,
    1.5e-4 m and 3.7e-7 from ground truth: the rounding of Z, not the optimiser (printed below, not asserted)."""
    k = pc.kitti_case(True, np.float64)
    r = _run(ref.optimize, k, damping=0.0, max_iterations=10, epsilon=1e-3)
    dt, dq = pc.pose_difference(r["X"], k["truth"])
    print("float64 Z: iterations %d chi %s final %.3g |dt| %.3g |dq| %.3g" % (r["iterations"], ["%.3g" % c for c in r["chi"]], r["chi_final"], dt, dq))
    assert r["status"] == ref.OK and dt <= 1e-4 and dq <= 1e-6
    k32 = pc.kitti_case(True)
    r32 = _run(ref.optimize, k32, damping=0.0, max_iterations=10, epsilon=1e-3)
    print("float32 Z: chi_final %.3g |dt| %.3g |dq| %.3g" % ((r32["chi_final"],) + pc.pose_difference(r32["X"], k32["truth"])))


def test_shipped_damping_creeps_but_never_increases_chi():
    k = pc.kitti_case(True)
    r = _run(ref.optimize, k, damping=1e-6, max_iterations=10, epsilon=0.0)
    chi = r["chi"] + [r["chi_final"]]
    assert r["iterations"] == 10 and all(b <= a for a, b in zip(chi, chi[1:])), chi


def test_termination_rule():
    c = pc.case("ring8")
    free = _run(ref.optimize, c, damping=0.0, max_iterations=8, epsilon=0.0)
    assert free["iterations"] == 8 and len(free["chi"]) == 8
    assert _run(ref.optimize, c, damping=0.0, max_iterations=8, epsilon=-1.0)["iterations"] == 8
    eps = 1e-3
    chi = free["chi"]
    ratios = [(chi[i - 1] - chi[i]) / chi[i - 1] for i in range(1, len(chi))]
    stop = next(i for i, q in enumerate(ratios, start=1) if q < eps)
    # the case separates the rule from rounding: no decay ratio up to the stop lies within a factor 2 of epsilon
    assert all(not (eps / 2 <= q <= 2 * eps) for q in ratios[:stop]), ratios
    r = _run(ref.optimize, c, damping=0.0, max_iterations=8, epsilon=eps)
    assert r["iterations"] == stop and len(r["chi"]) == stop + 1
    assert r["chi"] == chi[: stop + 1]


@pytest.fixture(scope="module")
def dense_runs():
    out = {}
    for c in pc.cases() + (pc.kitti_case(),):
        out[c["name"]] = (_run(ref.optimize, c, damping=0.0, max_iterations=5, epsilon=0.0),
                          _run(ref.optimize_dense, c, damping=0.0, max_iterations=5, epsilon=0.0))
    return out


def test_restatement_against_dense(dense_runs):
    """every case, criterion off, 5 iterations, damping 0 (Gauss-Newton converges, so what is left is the two solvers' rounding):
    the largest |dt| and |dq| are printed; pose_graph_cases.MEASURED_* hold them and 10 x that is the bound"""
    worst_t = worst_q = 0.0
    for name, (a, b) in dense_runs.items():
        assert a["status"] == b["status"] == ref.OK and a["iterations"] == b["iterations"], name
        dt, dq = pc.pose_difference(a["X"], b["X"])
        print("%-22s |dt| %.3g |dq| %.3g chi_final %.6g / %.6g" % (name, dt, dq, a["chi_final"], b["chi_final"]))
        worst_t, worst_q = max(worst_t, dt), max(worst_q, dq)
    print("largest |dt| %.3g |dq| %.3g" % (worst_t, worst_q))
    assert worst_t <= 10 * pc.MEASURED_MAX_DT and worst_q <= 10 * pc.MEASURED_MAX_DQ


def test_graph_groups_equal_the_reference_files():
    from srrg2_proslam_amd import configs
    with open(os.path.join(pc.GOLDEN, "ref_conf_graph.json")) as f:
        golden = json.load(f)
    for name, cfg in configs.CONFIGS.items():
        mine, group = cfg["graph"], golden[name]
        assert group["closure_validator"] == 0 and mine["algorithm"] == group["algorithm"], name
        assert [mine["max_iterations"]] == group["max_iterations"] and mine["epsilon"] == group["epsilon"], name
        if "damping" in group:  # (the LM files have none: configs._graph)
            assert mine["damping"] == group["damping"], name
    # malaga is read too (no hot-path group of its own): the same solver as kitti
    assert golden["malaga"] == golden["kitti"]
