"""The closure merger's rule (tests/closure_merge_ref.py, the numpy restatement of include/proslam_hip.h "Closure merger") against
the two results the reference pins for the base merge on its ICL frames (tests/test_mergers.cpp:174-246), the cap and the binning
at work on the same frames, properties of the rule, the synthetic cases the GPU suite replays, and the shipped configurations'
closure_merger groups.  No GPU."""
import json
import os

import numpy as np
import pytest

import closure_merge_cases as cc
import closure_merge_ref as cr
import ref_pins as rp
from test_ref_pins import OracleBackend


@pytest.fixture(scope="module")
def B():
    return OracleBackend()


def test_fixture_sizes(B):
    d = cc.icl(B)
    assert d["scene"]["n_points"] == 321 and len(d["meas"][("01", cr.UVD)]) == 338 and len(d["corr"]["01"]) == 282


@pytest.mark.parametrize("kind", [cr.UVD, cr.XYZ])
def test_reference_pin_00_to_00(B, kind):
    """321 points stay 321 and nothing moves beyond 1e-5 (tests/test_mergers.cpp:194-204)"""
    c = cc.icl_case(B, "00", 0.25, 1000, 1, kind)
    S, res, _ = cc.want(c)
    assert res == (321, 0, cr.OK) and S["n_points"] == 321
    assert np.abs(S["coords"][:321, :3] - c["scene"]["coords"][:321, :3]).max() <= 1e-5


@pytest.mark.parametrize("kind", [cr.UVD, cr.XYZ])
def test_reference_pin_00_to_01(B, kind):
    """321 points become 431 with 338 measurements, every old point within 0.25 per coordinate (tests/test_mergers.cpp:229-245)"""
    c = cc.icl_case(B, "01", 0.25, 1000, 1, kind)
    S, res, info = cc.want(c)
    assert res == (228, 110, cr.OK) and S["n_points"] == 431
    moved = np.abs(S["coords"][:321, :3] - c["scene"]["coords"][:321, :3]).max()
    print("largest coordinate change %.4f" % moved)
    assert moved <= 0.25
    assert len(info["merged"]) == 228 and not set(info["merged"]) & set(info["added"])


@pytest.mark.parametrize("frame,distance2,target,binning,wanted", cc.ICL_CASES)
def test_cap_on_the_icl_frames(B, frame, distance2, target, binning, wanted):
    S, res, info = cc.want(cc.icl_case(B, frame, distance2, target, binning))
    assert (S["n_points"], res[0], res[1]) == wanted and res[2] == cr.OK
    assert res[0] + res[1] <= max(target, res[0])  # the cap is honoured


@pytest.mark.parametrize("target", [250, 300])
def test_binning_decides_which_candidates_are_taken(B, target):
    on = cc.want(cc.icl_case(B, "01", 0.01, target, 1))[2]
    off = cc.want(cc.icl_case(B, "01", 0.01, target, 0))[2]
    assert len(on["added"]) == len(off["added"]) and set(on["added"]) != set(off["added"])
    bins = on["bins"][on["pass1"]]
    assert len(bins) > 0 and (bins >= 0).all() and len(set(bins)) == len(bins)  # no two pass-1 picks share a bin
    blocked = set(on["bins"][on["merged"]])
    assert not blocked & set(bins)
    # without binning: the first candidates in measurement order
    unmerged = [m for m in range(338) if m not in set(off["merged"])]
    assert list(off["added"]) == unmerged[: len(off["added"])]


def test_result_does_not_depend_on_the_order_of_the_vector(B):
    c = dict(cc.icl_case(B, "01", 0.01, 250, 1))
    S0, r0, _ = cc.want(c)
    rng = np.random.default_rng(5)
    for _ in range(3):
        c["corr"] = c["corr"][rng.permutation(len(c["corr"]))]
        S, r, _ = cc.want(c)
        assert r == r0 and cr.scenes_equal(S, S0)
    e = dict(cc.edge("pass1_longer_than_cap"))
    S0, r0, _ = cc.want(e)
    e["corr"] = e["corr"][::-1].copy()
    S, r, _ = cc.want(e)
    assert r == r0 and cr.scenes_equal(S, S0)


@pytest.mark.parametrize("target", [0, 1, 40, 41, 42, 60, 128, 129, 1000])
def test_cap_is_never_exceeded(target):
    c = dict(cc.edge("xyz_all"))
    c["P"] = dict(c["P"], target_number_of_merges=target)
    S, r, info = cc.want(c)
    assert r[2] == cr.OK and S["n_points"] == 100 + r[1]
    assert r[1] == (max(min(target - r[0], 128 - r[0]), 0) if r[0] < target else 0)
    assert r[0] + r[1] <= max(target, r[0])


def test_invalid_depth_is_never_merged_or_added():
    c = cc.edge("invalid_depths")
    S, r, info = cc.want(c)
    d = c["measurement"][:, 2]
    bad = set(np.nonzero(~(np.isfinite(d) & (d > 0)))[0])
    assert len(bad) == 30 and not bad & set(info["added"]) and not bad & set(info["merged"])
    assert np.isfinite(S["coords"][: S["n_points"], :3]).all()


@pytest.mark.parametrize("name", sorted(cc.EDGES))
def test_synthetic_case_is_what_its_name_says(name):
    c = cc.edge(name)
    S, r, info = cc.want(c)
    assert c["check"](r, info, c), (name, r, len(info["pass1"]), info["n_winners"], info["n_to_add"])
    # what the rule never touches
    n0, n1 = c["scene"]["n_points"], S["n_points"]
    assert np.array_equal(S["coords"][:n0, 3], c["scene"]["coords"][:n0, 3])
    for k in S:
        if k != "n_points":
            assert S[k][n1:].tobytes() == c["scene"][k][n1:].tobytes(), k


@pytest.mark.parametrize("name", sorted(cc.SIZES))
def test_size_case_is_what_its_name_says(name):
    """the cases of a bitmap word per thread (tests/test_closure_merge_sizes_gpu.py replays them on the device)"""
    c = cc.size(name)
    S, r, info = c["want"]
    assert c["check"](r, info, c), (name, r, len(info["pass1"]), info["n_winners"], info["n_to_add"], cc.n_candidates(info, c),
                                    list(cc.per_wave(info["added"])), list(cc.per_wave(info["pass1"])))
    n0, n1 = c["scene"]["n_points"], S["n_points"]
    assert n1 == n0 + r[1] <= c["scene"]["coords"].shape[0]
    assert np.array_equal(S["coords"][:n0, 3], c["scene"]["coords"][:n0, 3])
    for k in S:
        if k != "n_points":
            assert S[k][n1:].tobytes() == c["scene"][k][n1:].tobytes(), k


def test_shared_measurement_undercounts_the_candidates():
    """ten landmarks merge with one measurement: n_measured - n_merged caps the additions below the number of candidates although the
    target is far away (here 133 candidates for at most 125 places)"""
    c = cc.size("shared_measurement")
    _, r, info = c["want"]
    n_cand = cc.n_candidates(info, c)
    assert r[1] == info["n_to_add"] == 200 - r[0] < n_cand and r[0] + n_cand < 1000
    assert r[0] - len(info["merged"]) >= 5  # most of the ten share the measurement (a response >= 50 keeps one out)


def test_half_bins_sit_where_the_two_roundings_part():
    c = cc.size("half_bins")
    z = c["measurement"]
    assert np.array_equal(z[:, 0] % 8, np.full(400, 4, np.float32)) and np.array_equal(z[:, 1] % 8, np.full(400, 4, np.float32))
    assert cc.rint_bins_differ(c["want"][2], c) > 200


def test_mixed_group_shares_what_a_launch_shares():
    cases = cc.mixed_group()
    assert [len(c["measurement"]) for c in cases] == [16384, 4097, 1, 0, 16384]
    assert all(c["P"] == cases[0]["P"] and len(c["scene"]["coords"]) == 5000 + 16384 for c in cases)
    results = [c["want"][1] for c in cases]
    assert all(r[2] == cr.OK for r in results) and results[3] == (0, 0, cr.OK) and results[2][0] + results[2][1] == 1
    # with the group's parameters the two full pairs still use every wave, and pass 1 as well as pass 2
    for c in (cases[0], cases[4]):
        info = c["want"][2]
        assert (cc.per_wave(info["added"]) > 0).all() and 0 < len(info["pass1"]) < len(info["added"])


def test_size_error_cases_report_the_first_fault():
    items = cc.error_batch_sizes()
    assert [code for _, code in items] == [cr.ERR_DUPLICATE, cr.ERR_RANGE, cr.OK]
    for c, code in items:
        S, r, _ = c["want"]
        assert r[2] == code and len(c["corr"]) == len(c["measurement"]) == 16384
        if code != cr.OK:
            assert r[:2] == (0, 0) and cr.scenes_equal(S, c["scene"])
        else:
            assert r[0] > 256 * 5 and r[1] > 0


def test_error_cases_report_the_first_fault():
    for c, kw, code in cc.error_batch():
        S, r, _ = cc.want(c, **kw)
        assert r[2] == code
        if code in (cr.ERR_RANGE, cr.ERR_CAPACITY, cr.ERR_DUPLICATE):
            assert r[:2] == (0, 0) and cr.scenes_equal(S, c["scene"])
        elif code == cr.ERR_SCENE_FULL:
            n = c["scene"]["n_points"]
            assert r[0] > 0 and r[1] == 0 and S["n_points"] == n and not cr.scenes_equal(S, c["scene"])
            for k in S:
                if k != "n_points":
                    assert S[k][n:].tobytes() == c["scene"][k][n:].tobytes(), k


def test_closure_merger_groups_equal_the_reference_files():
    from srrg2_proslam_amd import configs
    with open(os.path.join(rp.GOLDEN, "ref_conf_closure.json")) as f:
        golden = json.load(f)
    assert sorted(golden) == ["euroc", "icl", "kitti", "malaga", "tum"]
    for name, g in golden.items():
        assert g == {"class": "MergerCorrespondencePointIntensityDescriptor3f", "enable_binning": 1, "maximum_distance_geometry_squared": 0.25,
                     "maximum_response": 50, "target_number_of_merges": 200}, name
    for name, cfg in configs.CONFIGS.items():
        group = cfg["closure_merger"]
        for k, v in golden[name].items():
            if k != "class":
                assert group[k] == v, (name, k)
        assert (group["number_of_row_bins"], group["number_of_col_bins"]) == (10, 30)  # merger_projective.h:47-56


def test_formats_follows_the_slice_pointer():
    from srrg2_proslam_amd import formats
    text = '''
"MergerCorrespondencePointIntensityDescriptor3f" { "#id" : 7, "enable_binning" : 0, "maximum_response" : 12, "target_number_of_merges" : 3 }
"TrackerSliceProcessorStereoProjective" { "#id" : 2, "name" : "slice", "closure_merger" : { "#pointer" : 9 }, "merger" : { "#pointer" : 7 } }
"MergerCorrespondencePointIntensityDescriptor3f" { "#id" : 9, "enable_binning" : 1, // a comment
  "maximum_distance_geometry_squared" : 0.5, "maximum_response" : 40, "target_number_of_merges" : 100 }
'''
    got = formats.closure_merger_params(formats.parse_conf(text))
    assert got == {"class": "MergerCorrespondencePointIntensityDescriptor3f", "enable_binning": 1, "maximum_distance_geometry_squared": 0.5,
                   "maximum_response": 40, "target_number_of_merges": 100}
    assert formats.closure_merger_params(formats.parse_conf('"Other" { "#id" : 1 }')) == {}
    assert formats.closure_merger_params(formats.parse_conf('"Slice" { "#id" : 1, "closure_merger" : { "#pointer" : -1 } }')) == {}
