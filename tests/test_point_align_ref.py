"""The loop aligner's CPU checker (tests/point_align_ref.py) against float64, the reference's loop-closing gtests and the
shipped configurations (no GPU needed)."""
import json
import os

import numpy as np
import pytest

import point_align_ref as par
from oracle import binding as ob
from srrg2_proslam_amd import configs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def backend():
    import __graft_entry__ as g
    g.build()
    from test_ref_pins import OracleBackend
    return OracleBackend()


def synthetic(rng, n, outliers=0.3, noise=0.01):
    """moving cloud, fixed = T moving + noise with a share of wrong partners; T = movingInFixed"""
    moving = rng.uniform(-10, 10, (n, 3)).astype(np.float32) + np.float32([0, 0, 15])
    T = ob.tnq2t(np.array([0.3, -0.2, 0.5, 0.02, -0.03, 0.05], np.float32)).astype(np.float64)
    fixed = (moving.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rng.normal(0, noise, (n, 3))).astype(np.float32)
    corr = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    bad = rng.random(n) < outliers
    corr[bad, 1] = rng.integers(0, n, bad.sum())
    return fixed, moving, corr, T


GUESS = ob.tnq2t(np.array([0.28, -0.18, 0.48, 0.019, -0.028, 0.048], np.float32))


@pytest.mark.parametrize("form", [par.CLAMP, par.SATURATED])
def test_single_linearisation_against_float64(form):
    rng = np.random.default_rng(3)
    fixed, moving, corr, T = synthetic(rng, 300)
    P = par.params(robustifier=form, chi_threshold=1.0)
    X = ob.tnq2t(np.array([0.25, -0.1, 0.45, 0.015, -0.02, 0.04], np.float32))
    lin = par.linearize(P, X, fixed, moving, corr)
    H64, b64, chi64, n64 = par.linearize_f64(P, X, fixed, moving, corr)
    assert lin["num_inliers"] == n64
    # 300 float32 terms of size |y|^2 ~ 4e2 summed: a relative error of a few 1e-6 of the largest entry is the float32 budget
    assert np.abs(lin["H"] - H64).max() <= 1e-5 * np.abs(H64).max()
    assert np.abs(lin["b"] - b64).max() <= 1e-5 * np.abs(H64).max()
    assert abs(float(lin["chi_inliers"]) - chi64) <= 1e-5 * max(chi64, 1.0)


@pytest.mark.parametrize("form", [par.CLAMP, par.SATURATED])
@pytest.mark.parametrize("n", [5, 64, 257, 2000])
def test_loop_pose_against_float64(form, n):
    rng = np.random.default_rng(n)
    fixed, moving, corr, T = synthetic(rng, n)
    P = par.params(robustifier=form, chi_threshold=1.0, max_iterations=20, min_num_inliers=3)
    X0 = GUESS
    X, res, _ = par.align(P, X0, fixed, moving, corr)
    X64 = par.align_f64(P, X0, fixed, moving, corr)
    assert np.linalg.norm(X - X64) / np.linalg.norm(X64) <= 1e-4
    assert res["iterations"] == 20 and res["num_inliers"] >= 0.6 * n


@pytest.mark.parametrize("form", ["clamp", "saturated"])
def test_reference_scenarios(backend, form):
    for sc in par.scenarios(backend):
        corr, _ = ob.bruteforce_match(sc["fixed_desc"], sc["moving_desc"], sc["max_distance"], 0.9)
        loop = dict(configs.get(sc["config"])["loop"], robustifier=form)
        X, res, _ = par.align(par.from_loop_group(loop), np.eye(4), sc["fixed"], sc["moving"], corr)
        assert res["status"] == 1 and res["accepted"] == 1, (sc["name"], res)
        if sc["truth"] is None:
            assert np.linalg.norm(par.pose_error(X, np.eye(4))) < 1e-5  # test_loop_closing.cpp:69
            assert len(corr) == 145 and res["num_inliers"] == 145
        else:
            err = par.pose_error(X, sc["truth"])
            assert (np.abs(err) < np.asarray(sc["bounds"])).all(), (sc["name"], err)


def test_unrelated_places_are_rejected(backend):
    for sc in par.unrelated(backend):
        corr, _ = ob.bruteforce_match(sc["fixed_desc"], sc["moving_desc"], sc["max_distance"], 0.9)
        assert len(corr) <= 3, sc["name"]
        X, res, _ = par.align(par.from_loop_group(configs.get(sc["config"])["loop"]), np.eye(4), sc["fixed"], sc["moving"], corr)
        assert res["accepted"] == 0 and res["status"] == 0, sc["name"]


def test_loop_groups_match_the_shipped_configurations():
    with open(os.path.join(GOLDEN, "ref_conf_loop.json")) as f:
        ref = json.load(f)
    for name in ("kitti", "euroc", "icl", "tum"):
        got, want = configs.get(name)["loop"], ref[name]
        for k in ("robustifier", "chi_threshold", "damping", "max_iterations", "min_num_inliers", "maximum_descriptor_distance",
                  "relocalize_min_inliers", "relocalize_min_inliers_ratio", "relocalize_max_chi_inliers"):
            assert got[k] == want[k], (name, k)
        assert got["min_num_correspondences"] == want.get("min_num_correspondences", 0), name
        assert got["relocalizer"] == want["relocalizer"], name
        # one Gauss-Newton iteration per aligner iteration, no inlier-only runs (what the kernel implements)
        assert want["solver_iterations"] == [1] and want["enable_inlier_only_runs"] == 0 and want["keep_only_inlier_correspondences"] == 0


def test_loop_params_reads_the_wiring():
    from srrg2_proslam_amd import formats
    text = '''"RobustifierSaturated" { "#id": 3, "chi_threshold": 0.5 }
"AlignerSliceProcessor3D" { "#id": 2, "min_num_correspondences": 7, "robustifier": { "#pointer": 3 } }
"IterationAlgorithmGN" { "#id": 5, "damping": 0.25 }
"Solver" { "#id": 4, "algorithm": { "#pointer": 5 }, "max_iterations": [1] }
"MultiAligner3DQR" { "#id": 1, "max_iterations": 12, "min_num_inliers": 9, "slice_processors": [{ "#pointer": 2 }], "solver": { "#pointer": 4 } }
"MultiLoopDetectorHBST3D" { "#id": 6, "maximum_descriptor_distance": 30, "relocalize_aligner": { "#pointer": 1 }, "relocalize_min_inliers": 11 }
'''
    got = formats.loop_params(formats.parse_conf(text))
    assert got == dict(maximum_descriptor_distance=30, relocalize_min_inliers=11, max_iterations=12, min_num_inliers=9,
                       min_num_correspondences=7, robustifier="saturated", chi_threshold=0.5, solver_iterations=[1], damping=0.25)
