"""The dense aligner's restatement (tests/dense_align_ref.py) on its own: that the rule it states aligns, that its system is the
Gauss-Newton system of the residual it states, that every class of sample occurs and is counted, and that its two statements of the
reduction agree.  No GPU needed; the device tests compare the kernels with this restatement byte for byte."""
import numpy as np
import pytest

import dense_align_cases as cases
import dense_align_ref as ref
from srrg2_proslam_amd import configs

F = np.float32
SCHEDULE = configs.DENSE_ALIGN["schedule"]
# planted offsets: (translation in metres, rotations in radians): 4 to 9 cm and 2.5 to 5 degrees in all
OFFSETS = (((0.03, -0.02, 0.025), (0.02, -0.03, 0.025)), ((-0.04, 0.03, -0.02), (-0.03, 0.02, -0.04)),
           ((0.05, 0.05, -0.05), (0.05, -0.05, 0.05)))
# Measured with this restatement over the three offsets, both depth types, with and without live normals (80 x 60 images, the
# default schedule): at most 0.49 mm and 0.20 mrad are left (f32: 0.03 .. 0.48 mm, 0.04 .. 0.19 mrad; u16 millimetres: 0.04 .. 0.49 mm,
# 0.05 .. 0.20 mrad).  The bounds are about twice that.
MAX_TRANSLATION, MAX_ROTATION = 1.0e-3, 4.0e-4


def settings(s, **kw):
    return ref.params(s["camera"], s["depth_type"], s["scale"], **kw)


def run(s, p, X0=None, normals=False, step=1):
    return ref.align(p, np.eye(4, dtype=F) if X0 is None else X0, s["model_depth"], s["model_normal"], s["live_depth"],
                     s["live_normal"] if normals else None, step)


@pytest.mark.parametrize("depth_type", ["f32", "u16"])
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("which", range(len(OFFSETS)))
def test_the_default_schedule_recovers_a_planted_offset(which, normals, depth_type):
    s = cases.pair(*OFFSETS[which], depth_type=depth_type)
    before = ref.pose_error(np.eye(4), s["X_true"])
    assert 0.04 < before[0] < 0.1 and 0.04 < before[1] < 0.1
    X, res, _ = ref.align_schedule(settings(s), np.eye(4), s["model_depth"], s["model_normal"], s["live_depth"],
                                   s["live_normal"] if normals else None, SCHEDULE)
    dt, dr = ref.pose_error(X, s["X_true"])
    print("offset %d normals %d %s: %.3g m, %.3g rad left" % (which, normals, depth_type, dt, dr))
    assert dt < MAX_TRANSLATION and dr < MAX_ROTATION
    assert res["status"] == 1 and res["iterations"] == SCHEDULE[-1][1] == res["steps_taken"] and res["num_inliers"] > 4000


@pytest.mark.parametrize("robustifier", [ref.CLAMP, ref.SATURATED])
def test_the_system_is_the_gauss_newton_system_of_the_residual(robustifier):
    """H and b of one linearisation against a float64 finite-difference Jacobian of r under X exp(dx) over the same weighted samples.
    Tolerance: a term is formed in float32 from float32 inputs in about ten roundings, and the fixed-shape sum of N terms adds
    log2(256 * P * 64) / 2 + P + chunks / 64 roundings to a term's path, under twenty in all here, so an entry of H or b is off by at
    most 30 eps of the sum of its terms' magnitudes, which is at most sqrt(H_ii H_jj) (Cauchy-Schwarz) and sqrt(H_ii chi_total'); the
    finite difference itself (h = 1e-6 on a residual linear in dt and quadratic in dq) is good to 1e-9 relative.  The assertion
    allows 1e-5 of those magnitudes, three times 30 eps."""
    s = cases.pair(*OFFSETS[0])
    X0 = cases.offset((0.01, 0.0, -0.01), (0.0, 0.01, 0.0))
    p = settings(s, robustifier=robustifier, chi_threshold=2e-4, linearize_only=1)
    lin = ref.linearize(p, X0, s["model_depth"], s["model_normal"], s["live_depth"], None, 1)
    assert lin["num_inliers"] > 500 and lin["num_outliers"] > 500
    H, b = ref.linearize_f64(p, X0, s["model_depth"], s["model_normal"], s["live_depth"], 1, lin["cls"])
    scale = np.sqrt(np.diag(H))
    assert (np.abs(lin["H"] - H) <= 1e-5 * np.outer(scale, scale)).all(), np.abs(lin["H"] - H) / np.outer(scale, scale)
    total = np.sqrt(float(lin["chi_inliers"]) + (lin["num_outliers"] if robustifier == ref.SATURATED else 0.0))  # sum w r^2
    assert (np.abs(lin["b"] - b) <= 1e-5 * scale * total).all(), np.abs(lin["b"] - b) / (scale * total)
    assert (lin["H"] == lin["H"].T).all() and np.linalg.eigvalsh(H).min() > 0
    if robustifier == ref.CLAMP:   # the outliers weigh nothing
        only = ref.linearize_f64(p, X0, s["model_depth"], s["model_normal"], s["live_depth"], 1, np.where(lin["cls"] == ref.INLIER, 1, 0))
        assert np.allclose(only[0], H, rtol=0, atol=0)


@pytest.mark.parametrize("depth_type", ["f32", "u16"])
@pytest.mark.parametrize("robustifier", [ref.CLAMP, ref.SATURATED])
def test_every_class_occurs_and_is_counted(robustifier, depth_type):
    s = cases.class_pair(depth_type=depth_type)
    p = settings(s, robustifier=robustifier, max_iterations=2)
    X, res, mask = run(s, p, normals=True)
    counts = [int((mask == c).sum()) for c in range(5)]
    assert counts == [res["num_unmatched"], res["num_inliers"], res["num_outliers"], res["num_rejected"], res["num_invalid"]]
    assert sum(counts) == res["num_samples"] == 4800
    assert res["num_unmatched"] > 400 and res["num_inliers"] > 1500 and res["num_outliers"] >= 10 and res["num_rejected"] > 800
    assert res["num_invalid"] > 50
    # both gates reject: without the live normals fewer samples are rejected
    assert 0 < run(s, p, normals=False)[1]["num_rejected"] < res["num_rejected"]
    with np.errstate(all="ignore"):
        assert np.isfinite(res["H"]).all() and np.isfinite(res["b"]).all() and res["chi_total"] > res["chi_inliers"] > 0
    assert np.isclose(res["chi_total"] - res["chi_inliers"], res["num_outliers"] * p["chi_threshold"], rtol=1e-4)


def test_the_robustifiers_differ_only_in_what_an_outlier_weighs():
    s = cases.class_pair()
    a = run(s, settings(s, robustifier=ref.CLAMP, linearize_only=1), normals=True)
    b = run(s, settings(s, robustifier=ref.SATURATED, linearize_only=1), normals=True)
    assert (a[2] == b[2]).all() and a[1]["num_outliers"] >= 10
    assert a[1]["chi_inliers"] == b[1]["chi_inliers"] and a[1]["chi_total"] == b[1]["chi_total"]
    assert not (a[1]["H"] == b[1]["H"]).all()
    assert (np.diag(b[1]["H"]) >= np.diag(a[1]["H"])).all()


def test_linearize_only_makes_one_linearisation_and_no_step():
    s = cases.pair(*OFFSETS[0])
    X0 = cases.offset((0.01, 0.0, -0.01), (0.0, 0.01, 0.0))
    X, res, _ = run(s, settings(s, linearize_only=1, max_iterations=0), X0)
    assert X.tobytes() == X0.tobytes() and (res["iterations"], res["steps_taken"], res["status"]) == (1, 0, 1)
    lin = ref.linearize(settings(s), X0, s["model_depth"], s["model_normal"], s["live_depth"], None, 1)
    assert res["H"].tobytes() == lin["H"].tobytes() and res["b"].tobytes() == lin["b"].tobytes()
    # the result holds the LAST linearisation: after one iteration it is the one at X0 although X has moved on
    X1, res1, _ = run(s, settings(s, max_iterations=1), X0)
    assert res1["H"].tobytes() == lin["H"].tobytes() and X1.tobytes() != X0.tobytes() and res1["steps_taken"] == 1


def test_too_few_inliers_keep_the_estimate():
    s = cases.pair(*OFFSETS[0])
    X0 = cases.offset((0.01, 0.0, -0.01), (0.0, 0.01, 0.0))
    X, res, _ = run(s, settings(s, min_num_inliers=4800, max_iterations=3), X0)
    assert 0 < res["num_inliers"] < 4800
    assert X.tobytes() == X0.tobytes() and (res["status"], res["iterations"], res["steps_taken"]) == (0, 3, 0)
    # a plane alone leaves three degrees free: a pivot is not positive and the estimate stays, although the inliers suffice
    flat, mn = np.full((60, 80), 2.5, F), np.zeros((60, 80, 4), F)
    mn[..., 2:] = (-1, 1)  # g = (0, 0, -1, -y1, y0, 0): three rows of H are exactly zero
    X, res, _ = ref.align(ref.params(cases.CAMERA, "f32", 1.0, max_iterations=2), np.eye(4), flat, mn, flat, None, 1)
    assert res["status"] == 1 and res["num_inliers"] == 4800 and res["steps_taken"] == 0 and X.tobytes() == np.eye(4, dtype=F).tobytes()
    assert res["H"][2, 2] == 4800 and not res["H"][0].any()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_an_estimate_that_is_not_finite_is_warned_about_and_kept(bad):
    s = cases.pair(*OFFSETS[0])
    for at in ((0, 0), (1, 3), (2, 2)):
        X0 = np.eye(4, dtype=F)
        X0[at] = bad
        X, res, mask = run(s, settings(s), X0)
        assert X.tobytes() == X0.tobytes() and res["warnings"] == ref.PRS_ERR_RANGE
        assert (res["iterations"], res["status"], res["num_samples"], res["num_unmatched"]) == (0, 0, 4800, 0) and not mask.any()
    X0 = np.eye(4, dtype=F)
    X0[3, 0] = bad                               # the bottom row is not looked at
    assert run(s, settings(s, max_iterations=1), X0)[1]["warnings"] == 0


@pytest.mark.parametrize("step", [1, 2, 3, 4, 7, 100])
def test_steps_that_do_not_divide_the_image(step):
    s = cases.pair(*OFFSETS[0], rows=41, cols=25)
    rows_s, cols_s, n, chunks = ref.shape_of(41, 25, step)
    assert (rows_s, cols_s) == (-(-41 // step), -(-25 // step)) and n == rows_s * cols_s
    p = settings(s, min_num_inliers=1, max_iterations=1)
    X, res, mask = run(s, p, step=step)
    assert res["num_samples"] == n == mask.size and res["num_inliers"] > 0
    # the samples are the pixels (vs * step, us * step): the same call on the subsampled LIVE image sees other pixels, so it
    # differs, but the classes of the samples whose live pixel holds no depth agree with the image
    live = s["live_depth"][::step, ::step].reshape(-1)
    assert (mask[live == 0] == ref.UNMATCHED).all()
    if step == 100:
        assert n == 1 and chunks == 1


def test_the_two_statements_of_the_reduction_agree_bit_for_bit():
    """41 x 25 samples at P = 4: a full chunk and a second one of a single sample; terms of mixed sign and magnitude so that the order
    of the additions shows"""
    s = cases.class_pair(rows=41, cols=25)
    p = settings(s, robustifier=ref.SATURATED)
    cls, T, M = ref.terms(p, np.eye(4, dtype=F), s["model_depth"], s["model_normal"], s["live_depth"], s["live_normal"], 1)
    assert T.shape == (29, 1025) and ref.shape_of(41, 25, 1)[3] == 2 and M[:, 1024].any()
    a, b = ref.reduce(T, M), ref.reduce_loop(T, M)
    assert a.tobytes() == b.tobytes()
    with np.errstate(all="ignore"):
        plain = np.where(M, T, F(0)).astype(np.float64).sum(1)
    assert np.allclose(a, plain, rtol=1e-4) and (a.astype(np.float64) != plain).any()   # an order, not the exact sum
    rng = np.random.default_rng(5)
    T = (rng.normal(size=(29, 70 * 1024 + 3)) * 10.0 ** rng.integers(-3, 4, (29, 70 * 1024 + 3))).astype(F)
    M = rng.random(T.shape) < 0.7
    assert ref.reduce(T[:3], M[:3]).tobytes() == ref.reduce_loop(T[:3], M[:3]).tobytes()     # 71 chunks: a lane adds two of them
