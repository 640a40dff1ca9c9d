"""Guesses for the Levenberg-Marquardt pose-graph tests: the cases of tests/pose_graph_cases.py pushed off their own guess, so that
the optimiser has to reject steps.  Built once per process and never modified by a test."""
import functools

import numpy as np

import pose_graph_cases as pc
import pose_graph_ref as ref

SEED = 7

# (case, (t_sigma, q_sigma), variable_damping): what the restatement does on each, shipped parameters, epsilon 1e-3, 10 rounds
# (tests/test_pose_graph_lm_ref.py::test_trial_traces asserts the properties)
REJECTING = (
    ("ring8", (5.0, 0.55), 1),            # a round of exactly one rejection
    ("fixed_not_first", (5.0, 0.55), 0),  # rounds of 4 and 2 consecutive rejections: nu doubles
    ("fixed_not_first", (8.0, 0.6), 1),   # a round of 2 consecutive rejections
)
ALL_ACCEPTED = ("n65", (5.0, 0.55), 1)
OVERFLOW_STALLS = ("n2_one_edge", "chain3")  # from their own guess: chi reaches 0, every later trial is rejected, lambda overflows

# Largest difference between pose_graph_lm_ref.optimize_lm (the kernel's operation order) and optimize_lm_dense over the compared
# cases of tests/test_pose_graph_lm_ref.py::test_restatement_against_dense (it prints both figures), shipped parameters, epsilon
# 1e-3, 10 rounds: measured on the CPU.  The test asserts 10 x these.
MEASURED_MAX_DT = 3.5e-6   # metres (fixed_not_first perturbed by (8, 0.6): 3.40e-6)
MEASURED_MAX_DQ = 5.6e-7   # quaternion units (the same case: 5.55e-7)


def perturb(case, t_sigma, q_sigma, seed=SEED):
    """a copy of the case with every free node's guess, in ascending index, right-multiplied by _rand_pose(rng, t_sigma, q_sigma);
    one default_rng(seed) serves the whole graph"""
    c = dict(case)
    rng = np.random.default_rng(seed)
    poses = c["poses"].copy()
    for i in range(len(poses)):
        if not c["fixed"][i]:
            poses[i] = ref.se3_mul(poses[i], pc._rand_pose(rng, t_sigma, q_sigma))
    c["poses"] = poses
    c["name"] = "%s_p%g_%g_s%d" % (case["name"], t_sigma, q_sigma, seed)
    return c


@functools.lru_cache(maxsize=None)
def perturbed(name, t_sigma, q_sigma, seed=SEED):
    """perturb() of the case `name` of tests/pose_graph_cases.py"""
    return perturb(pc.case(name), t_sigma, q_sigma, seed)


# the Gauss-Newton suite's graph whose block row is wider than the 194-block LDS buffer left at node_stride 1024: 200 nodes, closure
# (0, 199).  From (sigmas, seed) below the restatement rejects steps in two rounds of four: trials [1, 3, 3, 1]
WIDE_ROW_REJECTING = ((0.3, 0.25), SEED, 4)


@functools.lru_cache(maxsize=None)
def wide_row():
    return pc._graph("n200", np.random.default_rng(5), 200, closures=[(0, 199)], noise=(0.02, 0.004))


@functools.lru_cache(maxsize=None)
def wide_row_rejecting():
    sigmas, seed, _ = WIDE_ROW_REJECTING
    return perturb(wide_row(), *sigmas, seed)
