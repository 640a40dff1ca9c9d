"""The Levenberg-Marquardt pose-graph optimiser's float64 references (no GPU): the trial traces the reading produces (one rejection,
consecutive rejections, stall by lambda overflow, all accepted), the restatement against the dense implementation with the same
accept / reject decisions, the properties of the loop, and the C-ABI's new names and struct sizes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import pose_graph_cases as pc
import pose_graph_lm_cases as lc
import pose_graph_lm_ref as lm
import pose_graph_ref as ref

ROUNDS, EPS = 10, 1e-3


def run(c, fn=lm.optimize_lm, **over):
    return fn(c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], c["omega"], over, ROUNDS, EPS)


def min_abs_rho(w):
    r = [abs(x) for rr in w["rho"] for x in rr if x is not None]
    return min(r) if r else None


@pytest.fixture(scope="module")
def own_guess():
    return {c["name"]: run(c) for c in pc.cases()}


@pytest.fixture(scope="module")
def perturbed():
    runs = {}
    for name, sig, vd in lc.REJECTING + (lc.ALL_ACCEPTED,):
        c = lc.perturbed(name, *sig)
        runs[(name, sig, vd)] = (c, run(c, variable_damping=vd))
    return runs


def test_trial_traces(own_guess, perturbed):
    """seed 7, shipped parameters, epsilon 1e-3: the properties the prototype found, on the restatement (its `scale` is one chain, the
    prototype's was pairwise; every trace came out the same)"""
    traces = {k: w["trials"] for k, (c, w) in perturbed.items()}
    for k, t in traces.items():
        print(k, t, "min |rho| %.3g" % min_abs_rho(perturbed[k][1]))
    # a round of exactly one rejection (two trials)
    assert 2 in traces[lc.REJECTING[0]]
    # >= 2 consecutive rejections: nu doubled inside a round, and lambda grew by nu = 2 and then 4
    k = lc.REJECTING[1]
    w = perturbed[k][1]
    assert max(w["trials"]) >= 3
    it = int(np.argmax(w["trials"]))
    assert w["accepted"][it][:2] == [False, False]
    # (lambda entering the round is what the previous round left: its last lambda times the accept factor; the last trial solved with
    # lambda_in * 2 * 4 * ... = lambda_in * 2^(t (t - 1) / 2))
    t = w["trials"][it]
    assert w["lam"][it] > w["lam"][it - 1] * lm.SHIPPED["step_low"] * 2.0 ** (t * (t - 1) // 2) * (1 - 1e-6)
    assert max(traces[lc.REJECTING[2]]) >= 3
    # all accepted
    w = perturbed[lc.ALL_ACCEPTED][1]
    assert set(w["trials"]) == {1} and w["iterations"] == ROUNDS and w["stalled"] == 0 and min_abs_rho(w) >= 0.05
    # stalled by lambda overflow: every trial of the last round rejected, the last lambda is the largest finite one of the schedule
    for name in lc.OVERFLOW_STALLS:
        w = own_guess[name]
        print(name, w["trials"])
        assert w["status"] == ref.OK and w["stalled"] == 1 and w["rejected_not_positive_definite"] == 0
        assert 40 <= w["trials"][-1] < lm.SHIPPED["lm_iterations_max"] and not any(w["accepted"][-1])
        with np.errstate(over="ignore"):
            assert np.isfinite(w["lam"][-1]) and not np.isfinite(w["lam"][-1] * 2.0 ** w["trials"][-1])
        assert w["iterations"] == len(w["trials"]) - 1


def test_restatement_against_dense(own_guess, perturbed):
    """own guesses with min |rho| >= 0.01 and perturbed guesses with min |rho| >= 0.05: the same decisions in every trial, poses within
    10 x the measured difference (pose_graph_lm_cases.MEASURED_*)"""
    compared = [(pc.case(name), {}, 0.01) for name, w in own_guess.items() if w["rho"] and min_abs_rho(w) >= 0.01]
    assert sorted(c["name"] for c, _, _ in compared) == ["n130", "n65", "omega"]
    for k, (c, w) in perturbed.items():
        if min_abs_rho(w) >= 0.05:
            compared.append((c, dict(variable_damping=k[2]), 0.05))
    assert len(compared) == 6
    worst_t = worst_q = 0.0
    for c, over, floor in compared:
        a, b = run(c, **over), run(c, lm.optimize_lm_dense, **over)
        assert min_abs_rho(a) >= floor and min_abs_rho(b) >= floor, c["name"]
        assert a["accepted"] == b["accepted"] and a["trials"] == b["trials"], c["name"]
        assert a["status"] == b["status"] == ref.OK and a["iterations"] == b["iterations"] and a["stalled"] == b["stalled"], c["name"]
        dt, dq = pc.pose_difference(a["X"], b["X"])
        print("%-32s |dt| %.3g |dq| %.3g chi_final %.6g / %.6g" % (c["name"], dt, dq, a["chi_final"], b["chi_final"]))
        worst_t, worst_q = max(worst_t, dt), max(worst_q, dq)
    print("largest |dt| %.3g |dq| %.3g" % (worst_t, worst_q))
    assert worst_t <= 10 * lc.MEASURED_MAX_DT and worst_q <= 10 * lc.MEASURED_MAX_DQ


def test_properties(own_guess, perturbed):
    runs = list(own_guess.items()) + [(c["name"], w) for c, w in perturbed.values()]
    for name, w in runs:
        # chi[] holds accepted states only
        assert all(b <= a for a, b in zip(w["chi"], w["chi"][1:])), name
        assert w["chi_final"] <= w["chi"][0] if w["chi"] else w["chi_final"] == 0.0, name
        assert w["trials_total"] == sum(w["trials"]) and len(w["lam"]) == len(w["trials"]), name
    # a stalled run returns X0 exactly: the poses of the run that stops one round earlier
    for name in lc.OVERFLOW_STALLS:
        c, w = pc.case(name), own_guess[name]
        earlier = lm.optimize_lm(c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], c["omega"], {}, w["iterations"], EPS)
        assert earlier["stalled"] == 0 and np.array_equal(earlier["X"].view(np.uint64), w["X"].view(np.uint64)), name
    # a trial cap below the rejections a round needs stalls it too, at the guess of that round
    k = lc.REJECTING[1]
    c, w = perturbed[k]
    it = int(np.argmax(w["trials"]))
    capped = run(c, variable_damping=k[2], lm_iterations_max=w["trials"][it] - 1)
    earlier = lm.optimize_lm(c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], c["omega"], dict(variable_damping=k[2]), it, EPS)
    assert capped["stalled"] == 1 and capped["iterations"] == it and capped["trials"][-1] == w["trials"][it] - 1
    assert np.array_equal(capped["X"].view(np.uint64), earlier["X"].view(np.uint64))
    # user_lambda_init > 0 is used as given (widened from float32)
    c = pc.case("ring8")
    w = run(c, user_lambda_init=0.25)
    assert w["lam"][0] == 0.25 and w["trials"][0] == 1
    assert run(c)["lam"][0] != 0.25


def test_gauss_newton_diverges_where_lm_converges():
    c = lc.perturbed("n65", 5.0, 0.55)
    g = ref.optimize(c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], c["omega"], 1e-6, ref.DAMPING_DIAG, ROUNDS, EPS)
    w = run(c)
    print("chi[0] %.6g  Gauss-Newton chi_final %.6g  LM chi_final %.6g" % (g["chi"][0], g["chi_final"], w["chi_final"]))
    assert g["chi_final"] > g["chi"][0]
    assert w["chi"][0] == g["chi"][0] and w["chi_final"] < 1e-3 * w["chi"][0]


def test_isolated_free_node():
    """a free node no edge reaches: h_rr = 0.  lambda * diag(H) cannot lift it (every trial fails on the pivot), lambda * I does"""
    c = dict(pc.case("chain3"))
    c.update(src=np.array([0], np.int32), dst=np.array([1], np.int32), Z=pc.case("chain3")["Z"][:1])
    w = run(c, variable_damping=1)
    assert w["status"] == ref.ERR_NOT_POSITIVE and w["rejected_not_positive_definite"] == w["trials_total"] > 0 and w["stalled"] == 0
    assert np.array_equal(w["X"], c["poses"])
    w = run(c, variable_damping=0)
    assert w["status"] == ref.OK and w["iterations"] > 0 and w["rejected_not_positive_definite"] == 0


def test_exported_symbols_and_struct_sizes():
    from srrg2_proslam_amd import _lib
    import __graft_entry__ as g
    g.build()
    lib = _lib.load()
    for name in ("prs_pose_graph_lm_workspace_bytes", "prs_pose_graph_lm_struct_sizes", "prs_pose_graph_optimize_lm_batch",
                 "prs_pose_graph_optimize_lm"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    sizes = (C.c_uint64 * 2)()
    lib.prs_pose_graph_lm_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(_lib.PoseGraphLmParams), C.sizeof(_lib.PoseGraphLmResult)] == [32, 680]
    assert lib.prs_version() == 104
    # the envelope as for Gauss-Newton, and 28 doubles per node of node_stride
    assert lib.prs_pose_graph_lm_workspace_bytes(3, 8, 21) == lib.prs_pose_graph_workspace_bytes(3, 8, 21) + 3 * 8 * 28 * 8
    assert lib.prs_pose_graph_lm_workspace_bytes(0, 8, 21) == 0


def test_lm_groups_equal_the_reference_files():
    from srrg2_proslam_amd import configs
    with open(os.path.join(pc.GOLDEN, "ref_conf_graph_lm.json")) as f:
        golden = json.load(f)
    for name, cfg in configs.CONFIGS.items():
        graph = cfg["graph"]
        assert graph.get("lm", {}) == golden[name], name
        assert (graph["algorithm"] == "IterationAlgorithmLM") == bool(golden[name]), name
    assert golden["icl"] == golden["tum"] == {k: v for k, v in lm.SHIPPED.items()} and golden["malaga"] == {}
