"""The CPU checker's landmark estimators and mergers against the float64 restatement of tests/mapping_ref.py, on the cases of
tests/merge_cases.py: local maps whose origin is far from the world's, so that world_in_local_map (landmark_estimator_base.hpp:54)
is not the identity.  tests/test_merge_dispatch_gpu.py applies the same checks, with the same constants, to the device's arrays.

The constants are twice the largest deviation of the CHECKER from the float64 values over this module's own cases, rounded up to
one significant digit (the device must equal the checker bit for bit, so the margin covers nothing but a later change of cases)."""
import numpy as np
import pytest

from oracle import binding as ob
from oracle import binding_mapping as om
from tests import mapping_ref as mr
from tests import merge_cases as mc

STATE_TOL = 4e-5       # metres; measured 1.56e-5 (stereo filter, states ~100 m from the world's origin: a float ulp there is 7.6e-6)
COVARIANCE_TOL = 2e-5  # measured 8.26e-6 (mono filter, identity measurement covariance); 9.0e-8 for the stereo / depth filters
COORDS_TOL = 5e-5      # metres; measured 2.16e-5 (coords against world_in_local_map_f64 @ state)
STEP_TOL = 1e-4        # metres; measured 4.81e-5: the float64 Gauss-Newton step at the smoother's final state
MAX_LEFT_OUT = 0.05   # share of a case's merged landmarks the float64 comparison may leave out (gate within 1e-3 of its threshold,
                      # float64 smoother out of iterations)

ROWS = [(kind, binning) for kind in mc.KINDS for binning in (0, 1)]


def run_checker(P, seq, capacity=1200, check=True, corr_stride=None):
    """merge every frame of `seq` with the checker -> (map, pose table, deviations, landmarks merged, per-frame map copies)"""
    m = seq.new_map(capacity)
    poses = om.pose_table(seq.n_frames)
    dev, merged, history = mr.Deviations(), 0, []
    for k in range(seq.n_frames):
        Tw, Ts, z, desc, corr = seq.inputs(k, m, corr_stride)
        before = m.copy()
        rc, res = om.merge(P, Tw, Ts, poses, k, m, z, desc, corr)
        assert rc == 0, (k, rc)
        merged += res.n_merged
        if check:
            mr.check_frame(P, before, m, poses, k, Tw, Ts, z, desc, corr, dev=dev)
        history.append((m.copy(), (res.n_merged, res.n_added, res.flags)))
    return m, poses, dev, merged, history


def assert_within(dev, what):
    print("%s: %r" % (what, dev))
    assert dev.state <= STATE_TOL, (what, "state", dev.state)
    assert dev.covariance <= COVARIANCE_TOL, (what, "covariance", dev.covariance)
    assert dev.coords <= COORDS_TOL, (what, "coords", dev.coords)
    assert dev.step <= STEP_TOL, (what, "smoother step", dev.step)
    assert dev.share_left_out() <= MAX_LEFT_OUT, (what, "left out", dev.left_out, dev.checked, dev.reasons)


@pytest.mark.parametrize("kind,binning", ROWS)
def test_checker_against_float64_off_the_world_frame(oracle, kind, binning):
    P = mc.merger_params(kind, binning)
    total = mr.Deviations()
    for b, seq in enumerate(mc.distinct_batch(kind)):
        m, poses, dev, merged, _ = run_checker(P, seq)
        assert_within(dev, "%s binning %d map %d" % (kind, binning, b))
        if not seq.no_corr:
            assert merged > 20 and dev.checked > 20, (b, merged, dev.checked)
        # the scene frame really is not the world frame
        n = m.n_points
        assert n > 0 and np.abs(m.coords[:n, :3] - m.state[:n, :3]).max() > 10.0
        total.merge(dev)
    if kind != "mono_ekf":
        assert total.added > 300
    assert total.checked > 300


@pytest.mark.parametrize("kind,binning", ROWS)
def test_scene_frame_changes_nothing_but_coords(oracle, kind, binning):
    """the same sequence merged with measurement_in_scene = measurement_in_world and with L^-1 * measurement_in_world: everything
    but `coords` is bit-identical, `coords` differ by L^-1"""
    P = mc.merger_params(kind, binning)
    worst = 0.0
    for seed in (7, 8):
        a = run_checker(P, mc.Sequence(kind, seed, 250, 5), check=False)
        w = run_checker(P, mc.Sequence(kind, seed, 250, 5, scene_is_world=True), check=False)
        L = mc.Sequence(kind, seed, 250, 5).L
        Li = np.linalg.inv(L)
        for (ma, ra), (mw, rw) in zip(a[4], w[4]):
            assert ra == rw and ma.n_points == mw.n_points
            n = ma.n_points
            for name in ("state", "covariance", "n_opt", "inlier", "n_meas", "desc", "meas"):
                assert np.array_equal(getattr(ma, name)[:n].view(np.uint8), getattr(mw, name)[:n].view(np.uint8)), name
            moved = mr.f64(mw.coords[:n, :3]) @ Li[:3, :3].T + Li[:3, 3]
            worst = max(worst, float(np.abs(mr.f64(ma.coords[:n, :3]) - moved).max()))
        assert np.array_equal(a[1].view(np.uint8), w[1].view(np.uint8))  # pose tables
        assert a[3] > 50
    print("%s binning %d: coords against L^-1 * coords(world scene) %.3g" % (kind, binning, worst))
    # two roundings of coords (one per run) on top of the float64 relation
    assert worst <= 2 * COORDS_TOL, worst


def test_float64_reference_notices_a_wrong_scene_transform(oracle):
    """the check has teeth: coords written with the operands of world_in_local_map swapped miss COORDS_TOL by metres"""
    P = mc.merger_params("weighted_mean", 0)
    seq = mc.Sequence("weighted_mean", 3, 200, 3)
    m = seq.new_map(600)
    poses = om.pose_table(3)
    for k in range(2):
        Tw, Ts, z, desc, corr = seq.inputs(k, m)
        before = m.copy()
        assert om.merge(P, Tw, Ts, poses, k, m, z, desc, corr)[0] == 0
    t = mr.set_transforms(Tw, Ts)
    wrong = t["world_in_sensor"] @ t["sensor_in_local_map"]
    merged = np.nonzero(m.n_opt[: m.n_points] > 0)[0]
    assert len(merged) > 20
    for s in merged:
        m.coords[s, :3] = mr.apply(wrong, m.state[s, :3])
    dev = mr.check_frame(P, before, m, poses, 1, Tw, Ts, z, desc, corr)
    assert dev.coords > 1.0
