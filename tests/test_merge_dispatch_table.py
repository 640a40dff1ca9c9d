"""The parity table of tests/test_merge_dispatch_gpu.py names every kernel the merger can launch, and the library's own plan
(prs_merge_plan) picks each row's kernel sequence from the row's knobs (no GPU needed): a merge_kernel instantiation or smoother
kernel in the variant table without a row, a stale row, or a row whose knobs select other kernels fails here."""
import csv
import os

import pytest

from srrg2_proslam_amd import _lib, ops
from tests import merge_cases as mc
from test_merge_dispatch_gpu import DISPATCH, ERR_UNSUPPORTED, gpu_params, lds_request, row_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTHER_KERNELS = {"prs::smoother_kernel(prs::MergeArgs)", "prs::smoother_tail_kernel(prs::MergeArgs)"}


def enumerated():
    return ops.dispatch_kernel_names(_lib.DISPATCH_MERGE)


def table():
    return {k for row in DISPATCH for k in row_kernels(row)}


def plan(row, batch=6, capacity=1600, max_frames=5, history=True, params=None, **env):
    """prs_merge_plan for a row's knobs, as tests/test_merge_dispatch_gpu.py sets them up"""
    d = _lib.MergeBatch(batch=batch, capacity=capacity, max_measurements=8, max_frames=max_frames, measurement_stride=512, corr_stride=1024)
    d.corr = 64  # set, never followed
    if history:
        d.meas = 64
    return ops.merge_plan(gpu_params(params or mc.merger_params(row["kind"], 1)), d, ops.dispatch_env(merge_fused=row["fused"], **env))


def test_variant_table_holds_every_kernel():
    found = enumerated()
    assert len(found) == len(set(found))
    assert sum("::merge_kernel<" in n for n in found) == 7
    assert {n for n in found if "::merge_kernel<" not in n} == SMOOTHER_KERNELS


def test_every_dispatched_kernel_has_a_row():
    missing = set(enumerated()) - table()
    assert not missing, "kernels without a row in DISPATCH: %s" % sorted(missing)


def test_every_row_names_a_dispatched_kernel():
    stale = table() - set(enumerated())
    assert not stale, "rows naming no kernel of the dispatch: %s" % sorted(stale)
    assert all(row["merge"] for row in DISPATCH)


def test_the_kept_kernel_trace_lists_every_kernel():
    """profiles/merge_dispatch/kernel_stats.csv: the kernel trace of one run of the GPU module on an MI355X"""
    with open(os.path.join(ROOT, "profiles", "merge_dispatch", "kernel_stats.csv"), newline="") as f:
        traced = {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}
    assert all(traced.get(k, 0) > 0 for k in enumerated()), sorted(set(enumerated()) - set(traced))


def test_row_ids_are_unique():
    ids = [r["id"] for r in DISPATCH]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("row", DISPATCH, ids=[r["id"] for r in DISPATCH])
def test_row_is_chosen_by_its_knobs(row):
    p = plan(row)
    assert p["status"] == 0 and p["kernels"] == row_kernels(row), p
    assert p["split"] == (len(row_kernels(row)) == 4)
    for l in p["launches"]:
        tail = l["kernel"] == "prs::smoother_tail_kernel(prs::MergeArgs)"
        assert (l["grid_x"], l["grid_y"]) == (6, 1) and l["block"] == (64 if l["kernel"] in SMOOTHER_KERNELS else 256) and (l["lds"] == 0) == tail, l


@pytest.mark.parametrize("row", DISPATCH, ids=[r["id"] for r in DISPATCH])
def test_lds_request_and_its_refusal(row):
    """the dynamic LDS of the merge kernels is what tests/test_merge_dispatch_gpu.py::lds_request restates, up to 160 KiB"""
    for r, c in ((20, 60), (60, 80), (4, 6)):
        p = plan(row, capacity=256, max_frames=4, params=mc.merger_params(row["kind"], 1, row_bins=r, col_bins=c, target_merges=0))
        assert p["status"] == 0 and (p["nbr"], p["nbc"]) == (r + 2, c + 2)
        assert {l["lds"] for l in p["launches"] if "::merge_kernel<" in l["kernel"]} == {lds_request(row, 256, 4, r, c)}
    def widest(rb):
        return max(c for c in range(1, 4096) if lds_request(row, 256, 4, rb, c) <= 160 * 1024)
    # the fewest row bins whose widest accepted grid AND the next one still have columns of at least one pixel
    rb = min(r for r in range(2, 64) if widest(r) + 1 <= mc.camera(row["kind"])["cols"])
    at, over = (plan(row, capacity=256, max_frames=4, params=mc.merger_params(row["kind"], 1, row_bins=rb, col_bins=c, target_merges=0))
                for c in (widest(rb), widest(rb) + 1))
    assert at["status"] == 0 and max(l["lds"] for l in at["launches"]) == lds_request(row, 256, 4, rb, widest(rb))
    assert (over["status"], over["kernels"]) == (ERR_UNSUPPORTED, []) and over["message"].startswith("prs_merge_batch_run: bin table")


def test_smoother_knobs_and_refusals():
    split = next(r for r in DISPATCH if r["id"] == "smoother_split")
    assert plan(split, stamps=1)["kernels"] == ["void prs::merge_kernel<2, 4, 0>(prs::MergeArgs)"]  # (stamps time the one-kernel form)
    assert plan(split, batch=3000)["launches"][2]["grid_x"] == 2048 and plan(split, batch=2048)["launches"][2]["grid_x"] == 2048
    assert plan(split, batch=3000)["tail_capacity"] == 3000 * plan(split, batch=1)["tail_capacity"]
    no_history = plan(split, history=False)
    assert (no_history["status"], no_history["message"]) == (_lib.ERR_NULL, "prs_merge_batch_run: the pose-based smoother needs the measurement history")
    assert plan(split, batch=0) == dict(plan(split, batch=0), status=0, message=None, kernels=[])
