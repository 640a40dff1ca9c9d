"""tests/stereo_ref.py (a plain-Python restatement of the epipolar matcher) against the C oracle at the parameter edges the GPU tables
lean on and the reference's own gtests do not pin: distance thresholds 255 / 256, a second best of 0, ratios above one, multi-pass
pruning with thick epipolar lines, duplicate pixels and a maximum disparity of 0.  No GPU needed."""
import numpy as np
import pytest

import stereo_ref as sr
from helpers import oracle_stereo_params


def _both(oracle, fr, m):
    ref, flags = oracle.stereo_match(fr["uv_left"], fr["desc_left"], fr["uv_right"], fr["desc_right"], oracle_stereo_params(oracle, m))
    mine, my_flags = sr.match(fr["uv_left"], fr["desc_left"], fr["uv_right"], fr["desc_right"], m["maximum_descriptor_distance"],
                              m["maximum_distance_ratio_to_second_best"], m["minimum_matching_ratio"], m["maximum_disparity_pixels"],
                              m["epipolar_line_thickness_pixels"])
    return sr.as_tuples(ref), flags, mine, my_flags


def _params(**kw):
    m = {"maximum_descriptor_distance": 100.0, "maximum_distance_ratio_to_second_best": 0.8, "minimum_matching_ratio": 0.3,
         "maximum_disparity_pixels": 20, "epipolar_line_thickness_pixels": 0}
    m.update(kw)
    return m


def _far_windows(seed, dist_lists, rows=4):
    rng = np.random.default_rng(seed)
    fb = sr.FrameBuilder(rng)
    for k, dists in enumerate(dist_lists):
        fb.window(k % rows, 40 + 50 * (k // rows), dists, keep=bool(k % 3))
    return fb.build()


@pytest.mark.parametrize("max_dist", [254.0, 255.0, 255.5, 256.0, 256.5, 300.0])
def test_distance_thresholds(oracle, max_dist):
    lists = [[d] for d in (250, 253, 254, 255, 256)] + [[255, 256], [256, 255], [254, 256, 255], [256, 256], [255, 255, 256]]
    fr = _far_windows(1, lists * 4)
    ref, flags, mine, my_flags = _both(oracle, fr, _params(maximum_descriptor_distance=max_dist, maximum_distance_ratio_to_second_best=1.5))
    assert mine == ref and my_flags == flags
    assert max(r[2] for r in ref) == {254.0: 253.0, 255.0: 254.0, 255.5: 255.0, 256.0: 255.0, 256.5: 256.0, 300.0: 256.0}[max_dist]


@pytest.mark.parametrize("ratio", [0.5, 0.8, 1.0, 1.0001, 1.5, 3.0])
def test_second_best_zero_and_ratios_above_one(oracle, ratio):
    lists = [[0, 0], [0, 0, 0, 0, 0, 0], [5, 5], [0, 7], [9, 9, 9], [3, 2], [1, 0, 0], [7, 10], [8, 10], [6, 10, 30, 40, 50], [0]]
    fr = _far_windows(2, lists * 3)
    ref, flags, mine, my_flags = _both(oracle, fr, _params(maximum_distance_ratio_to_second_best=ratio))
    assert mine == ref and my_flags == flags
    # best 0 with second 0 is 0 / 0: never accepted ([0, 7] and [0] are, three times each); equal best and second are accepted iff
    # the ratio exceeds one
    assert sum(1 for r in ref if r[2] == 0.0) == 6
    n_equal = sum(1 for r in ref if r[2] in (5.0, 9.0))
    assert (n_equal > 0) == (ratio > 1.0)


@pytest.mark.parametrize("thickness", [1, 2, 5])
def test_multi_pass_pruning(oracle, thickness):
    rng = np.random.default_rng(10 + thickness)
    for k in range(3):
        fr = sr.crowded_frame(rng, 40, 12, 8, 10, 14, jitter=0.5, row_list=np.arange(10, 22), col0=200 + 10 * k)
        assert len(fr["uv_left"]) <= 300
        m = _params(maximum_disparity_pixels=14, epipolar_line_thickness_pixels=thickness)
        ref, flags, mine, my_flags = _both(oracle, fr, m)
        assert mine == ref and my_flags == flags
        _, _, passes = sr.match(fr["uv_left"], fr["desc_left"], fr["uv_right"], fr["desc_right"], 100.0, 0.8, 0.3, 14, thickness, passes=True)
        assert len(passes) == 1 + 2 * thickness and sum(len(p) for p in passes[1:]) > 0  # later passes match the pruned remainder


def test_duplicate_pixels_and_zero_disparity(oracle):
    rng = np.random.default_rng(3)
    n = 250
    uvl = np.stack([rng.integers(0, 40, n), rng.integers(0, 3, n)], axis=1).astype(np.float32) + 0.5
    uvr = np.stack([rng.integers(0, 40, n), rng.integers(0, 3, n)], axis=1).astype(np.float32) + 0.25
    bank = rng.integers(0, 256, (12, 32), dtype=np.uint8)
    dl = np.bitwise_xor(bank[rng.integers(0, 12, n)], np.packbits(rng.random((n, 256)) < 0.03, axis=1))
    dr = np.bitwise_xor(bank[rng.integers(0, 12, n)], np.packbits(rng.random((n, 256)) < 0.03, axis=1))
    fr = {"uv_left": uvl, "desc_left": dl, "uv_right": uvr, "desc_right": dr}
    for max_disp in (0, 1, 5, 100, -1):
        for thickness in (0, 1, 2):
            ref, flags, mine, my_flags = _both(oracle, fr, _params(maximum_disparity_pixels=max_disp, epipolar_line_thickness_pixels=thickness))
            assert mine == ref and my_flags == flags
            if max_disp == 0:
                assert ref and all(uvl[i, 0] // 1 == uvr[j, 0] // 1 for i, j, _ in ref)  # only candidates on the left's own column
            if max_disp < 0:
                assert not ref


def test_empty_and_lone_frames(oracle):
    e2, e32 = np.zeros((0, 2), np.float32), np.zeros((0, 32), np.uint8)
    fr = _far_windows(4, [[3], [4, 5]])
    for a in ({"uv_left": e2, "desc_left": e32, "uv_right": fr["uv_right"], "desc_right": fr["desc_right"]},
              {"uv_left": fr["uv_left"], "desc_left": fr["desc_left"], "uv_right": e2, "desc_right": e32},
              {"uv_left": e2, "desc_left": e32, "uv_right": e2, "desc_right": e32}, fr):
        ref, flags, mine, my_flags = _both(oracle, a, _params(minimum_matching_ratio=0.9))
        assert mine == ref and my_flags == flags
