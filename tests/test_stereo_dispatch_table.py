"""The parity table of tests/test_stereo_dispatch_gpu.py names every kernel instantiation the stereo matcher can dispatch to, and
tests/stereo_dispatch.py restates the host's limits and LDS layouts exactly as the library plans them (no GPU needed): an
instantiation in the library's variant tables without a parity row, a stale row, or a limit, carve or choice that the restatement
and prs_stereo_plan disagree on fails here."""
import csv
import itertools
import os

import pytest

import stereo_dispatch as sd
from srrg2_proslam_amd import _lib, ops
from test_stereo_dispatch_gpu import DISPATCH, M_KITTI, STANDALONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSALS = {"shape": "prs_stereo_match_batch: stride must be in [1,8192], image_rows in [1,4096]",
            "thickness": "prs_stereo_match_batch: epipolar_line_thickness_pixels > 120",
            "lds": "prs_stereo_match_batch: frame does not fit the 160 KiB LDS"}
V5_WHY = {None: 0, "stride": 1, "knob": 2, "cap": 3, "lds": 4, "best_lim": 5}


def enumerated():
    return ops.dispatch_kernel_names(_lib.DISPATCH_STEREO)


def table():
    return {sd.trace_name(r["kernel"], r["args"]) for r in DISPATCH} | {sd.TRIANGULATE_KERNEL for k in STANDALONE if k[0] == "triangulate_kernel"}


def plan(stride, rows, thickness, max_dist, epi, v3=0, unstaged=0, batch=1, cus=256):
    p = _lib.StereoParams(maximum_descriptor_distance=max_dist, epipolar_line_thickness_pixels=thickness, image_rows=rows)
    b = _lib.StereoBatch(batch=batch, stride=stride)
    if epi:  # set, never followed
        b.fixed_uvuv = b.fixed_desc = b.n_fixed = b.fixed_xyz = 64
        b.triangulator = _lib.C.pointer(_lib.TriangulatorParams())
    return ops.stereo_plan(p, b, ops.dispatch_env(cus=cus, matcher_v3=v3, force_unstaged=unstaged))


def test_variant_tables_hold_every_family():
    names = enumerated()
    assert sum("stereo_match5_kernel<" in n for n in names) == 8  # KPT 1 / 2 x MULTI x EPI
    assert sum("stereo_match_kernel<" in n for n in names) == 6   # staged KPT 1 / 2, unstaged KPT 1 / 2 / 4 / 8
    assert sd.TRIANGULATE_KERNEL in names
    assert len(names) == len(set(names)) == 15


def test_every_dispatched_instantiation_has_a_parity_row():
    missing = set(enumerated()) - table()
    assert not missing, "instantiations without a row in DISPATCH: %s" % sorted(missing)


def test_every_parity_row_names_a_dispatched_instantiation():
    stale = table() - set(enumerated())
    assert not stale, "rows naming no instantiation of the dispatch: %s" % sorted(stale)


def test_the_kept_kernel_trace_lists_every_kernel():
    """profiles/stereo_dispatch/kernel_stats.csv: the kernel trace of one run of the GPU module on an MI355X"""
    with open(os.path.join(ROOT, "profiles", "stereo_dispatch", "kernel_stats.csv"), newline="") as f:
        traced = {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}
    assert all(traced.get(k, 0) > 0 for k in enumerated()), sorted(set(enumerated()) - set(traced))


def test_row_ids_are_unique():
    ids = [r["id"] for r in DISPATCH]
    assert len(ids) == len(set(ids))


def test_every_row_is_chosen_by_its_knobs():
    for r in DISPATCH:
        knobs = (r["stride"], 376, r["thickness"], M_KITTI["maximum_descriptor_distance"], r["epi"], r.get("v3", 0), r.get("unstaged", 0))
        d = sd.dispatch(*knobs)
        assert (d["kernel"], d["args"]) == (r["kernel"], r["args"]), r["id"]
        assert plan(*knobs)["kernels"] == [sd.trace_name(r["kernel"], r["args"])], r["id"]
        assert max(r["n"]) == r["stride"] and len(set(r["n"])) == len(r["n"]), r["id"]  # a full frame, distinct counts


def check_against_plan(stride, rows, thickness, max_dist, epi, v3, unstaged, batch, cus):
    """the restatement and the library's plan, field by field"""
    what = (stride, rows, thickness, max_dist, epi, v3, unstaged, batch, cus)
    d = sd.dispatch(stride, rows, thickness, max_dist, epi, v3, unstaged, batch, cus)
    p = plan(*what)
    if d["refused"]:
        assert (p["status"], p["message"], p["launches"]) == (_lib.ERR_UNSUPPORTED, REFUSALS[d["refused"]], []), what
        if d["refused"] != "lds":
            return
    else:
        assert p["status"] == 0 and p["message"] is None, what
        launch, = p["launches"]
        assert launch == dict(kernel=sd.trace_name(d["kernel"], d["args"]), grid_x=d["grid"], grid_y=1, block=sd.KT,
                              lds=d["v5"]["lds"] if d["v5_why"] is None else d["staged_lds" if d["args"].endswith("true") else "unstaged_lds"]), what
    assert p["v5_why"] == V5_WHY[d["v5_why"]] and p["v5"] == (d["v5_why"] is None) and p["best_lim"] == sd.accept_limit(max_dist), what
    lay = d["v5"]
    if lay is not None:
        assert (p["cap"], p["v5_lds"]) == (lay["cap"], lay["lds"] or 0), what
        if lay["fits"]:
            assert (p["off_pool"], p["pool_cap"]) == (lay["off_pool"], lay["pool_cap"]), what
    if d["v5_why"] is not None:
        assert (p["staged_lds"], p["unstaged_lds"]) == (d["staged_lds"], d["unstaged_lds"]), what
        assert p["sort_cap"] == max(stride, rows + 1), what


STRIDES = (0, 1, 64, 1000, 1023, 1024, 1025, 2000, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)
ROWS = (0, 1, 17, 376, 480, 488, 489, 490, 491, 492, 493, 494, 2047, 2048, 2093, 2094, 2095, 2096, 4095, 4096, 4097)
THICKNESS = (0, 1, 119, 120, 121)
THRESHOLDS = (100.0, 254.5, 255.0, 255.5, 256.0, 256.5)


def test_restatement_equals_the_library_plan_over_a_sweep():
    """every limit and carve the restatement holds, at its edges and their neighbours (about 29 000 combinations)"""
    n = 0
    for stride, rows, epi, v3, unstaged in itertools.product(STRIDES, ROWS, (0, 1), (0, 1), (0, 1)):
        # the thickness and threshold edges do not interact: sweep each with the other at its usual value
        for thickness, max_dist in [(t, 100.0) for t in THICKNESS] + [(1, x) for x in THRESHOLDS[1:]]:
            check_against_plan(stride, rows, thickness, max_dist, epi, v3, unstaged, 4, 256)
            n += 1
    # the persistent grid: batch below / at / above the CU count, for every instantiation
    for stride, (v3, unstaged), batch, cus in itertools.product((1000, 2048, 4096, 8192), ((0, 0), (1, 0), (0, 1)), (1, 255, 256, 257, 1000), (256, 304, 8)):
        check_against_plan(stride, 376, 1, 100.0, 1, v3, unstaged, batch, cus)
        n += 1
    assert n > 25000


@pytest.mark.parametrize("stride,rows", [(1, 1), (64, 4096), (1000, 2094), (1000, 2095), (1024, 376), (2000, 376), (2048, 480), (2048, 489),
                                         (2048, 490), (2048, 493), (8192, 4096), (4097, 17)])
def test_restated_layouts_match_the_source_carves(stride, rows):
    """the restated v5 layout and first-generation carves against the ones the library computes (its plan), shape by shape"""
    lay = sd.v5_layout(stride, rows) if stride <= sd.V5_MAX_STRIDE else None
    p = plan(stride, rows, 0, 100.0, 1)
    if lay is not None:
        assert (p["cap"], p["v5_why"]) == (lay["cap"], V5_WHY[lay["why"]])
        if lay["why"] != "cap":
            assert p["v5_lds"] == lay["lds"]
        if lay["fits"]:
            assert (p["off_pool"], p["pool_cap"], p["launches"][0]["lds"]) == (lay["off_pool"], lay["pool_cap"], lay["lds"])
    # the first generation's two carves: what the library plans when v5 is switched off
    g = plan(stride, rows, 0, 100.0, 1, v3=1)
    assert (g["staged_lds"], g["unstaged_lds"]) == (sd.first_gen_carve(stride, rows, True), sd.first_gen_carve(stride, rows, False))


def test_layout_edges():
    """the shapes at which the pool and the v5 layout change, in the restatement and in the library's plan; the 13-bit cap never
    refuses a layout that would fit"""
    def both(stride, rows):
        lay, p = sd.v5_layout(stride, rows), plan(stride, rows, 0, 100.0, 1)
        assert (p["cap"], p["v5_why"]) == (lay["cap"], V5_WHY[lay["why"]]) and (not lay["fits"] or p["pool_cap"] == lay["pool_cap"])
        return lay
    assert both(2048, 489)["pool_cap"] == 64
    assert both(2048, 490)["pool_cap"] == 0 and both(2048, 492)["fits"]
    assert both(2048, 493)["why"] == "lds"
    assert both(1000, 2094)["pool_cap"] == 72 and both(1000, 2095)["pool_cap"] == 0
    assert both(2000, 376)["pool_cap"] == 3072
    assert both(2048, 480)["pool_cap"] == 248
    assert both(1024, 376)["pool_cap"] == sd.POOL_MAX
    assert both(2047, 2047)["cap"] == sd.V5_CAP_MAX and both(2048, 2048)["why"] == "cap"
    for stride in range(1, 2049, 31):
        for rows in range(stride - 40, stride + 3000, 97):
            if 1 <= rows <= sd.MAX_ROWS and (stride + 3 * min(rows, stride) + 3) & ~3 > sd.V5_CAP_MAX:
                assert both(stride, rows)["why"] == "cap"
                # the same layout without the cap check would not fit either: the arrays in front of the pool alone pass 160 KiB
                cap = (stride + 3 * min(rows, stride) + 3) & ~3
                assert stride * 40 + 20 * (cap + 4) + 20 * (rows + 2) > sd.LDS_LIMIT


def test_acceptance_table_edges():
    assert [sd.fill_accept_table(x, 0.5)[0] for x in (255.0, 255.5, 256.0, 256.5)] == [255, 256, 256, 257]
    assert [plan(1024, 376, 0, x, 0)["best_lim"] for x in (255.0, 255.5, 256.0, 256.5)] == [255, 256, 256, 257]
    lim, bmax = sd.fill_accept_table(100.0, 1.5)
    assert bmax[0] == -1 and bmax[1] == 1 and bmax[257] == 256
    _, bmax = sd.fill_accept_table(100.0, 0.8)
    assert bmax[10] == 7
