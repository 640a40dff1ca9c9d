"""The parity table of tests/test_align_dispatch_gpu.py names every kernel instantiation the aligner can dispatch to, and the
library's own plan (prs_align_plan) picks each row's kernels from the row's knobs (no GPU needed): an instantiation in the variant
table without a parity row, a stale row, a row whose knobs select another kernel, a moved max_fixed or batch threshold or a changed
survivor slot width fails here."""
import csv
import os

import pytest

from srrg2_proslam_amd import _lib, configs, ops
from test_align_dispatch_gpu import AK, DISPATCH, FRAMES_PER_ROW, FUSED_LIMIT, GN, SLOT_WIDTHS, _device_params, row_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def enumerated():
    return ops.dispatch_kernel_names(_lib.DISPATCH_ALIGN)


def table():
    return {k for row in DISPATCH for k in row_kernels(row)}


def plan(row, batch=FRAMES_PER_ROW, cus=256, max_fixed=None, stride=None, **env):
    """prs_align_plan for a row's knobs, as tests/test_align_dispatch_gpu.py sets them up"""
    fp, ap = _device_params(configs.get(row.get("cfg", "kitti")), row.get("fkw", {}), row.get("akw", {}), bool(row.get("sensor")), bool(row.get("mprior")))
    max_fixed = max_fixed or row["max_fixed"]
    d = _lib.AlignBatch(batch=batch, fixed_stride=stride or max_fixed, moving_stride=2048, max_fixed=max_fixed)
    return ops.align_plan(fp, ap, d, ops.dispatch_env(cus=cus, no_lone_gn=row.get("no_lone", 0), fused_align=row.get("fused", 0), **env))


def test_variant_table_holds_every_family():
    found = enumerated()
    assert len(found) == len(set(found))
    assert sum("::gn_kernel<" in n for n in found) == 14
    assert sum("::align_kernel<" in n for n in found) == 8  # 3 patterns x 2 slot widths, the KD-tree, the fused kernel


def test_every_dispatched_instantiation_has_a_parity_row():
    missing = set(enumerated()) - table()
    assert not missing, "instantiations without a row in DISPATCH: %s" % sorted(missing)


def test_every_parity_row_names_a_dispatched_instantiation():
    stale = table() - set(enumerated())
    assert not stale, "rows naming no instantiation of the dispatch: %s" % sorted(stale)


def test_the_kept_kernel_trace_lists_every_kernel():
    """profiles/align_dispatch/kernel_stats.csv: the kernel trace of one run of the GPU module on an MI355X"""
    with open(os.path.join(ROOT, "profiles", "align_dispatch", "kernel_stats.csv"), newline="") as f:
        traced = {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}
    assert all(traced.get(k, 0) > 0 for k in enumerated()), sorted(set(enumerated()) - set(traced))


def test_row_ids_are_unique():
    ids = [r["id"] for r in DISPATCH]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("row", DISPATCH, ids=[r["id"] for r in DISPATCH])
def test_row_is_chosen_by_its_knobs(row):
    p = plan(row)
    assert p["status"] == 0 and p["kernels"] == row_kernels(row), p
    assert p["split"] == (row["gn"] is not None) and p["max_fixed"] == row["max_fixed"]
    assert all(l["grid_x"] == FRAMES_PER_ROW and l["grid_y"] == 1 for l in p["launches"])
    assert [l["block"] for l in p["launches"]] == ([512, 128] if p["split"] else [256])
    if p["split"] and row["fkw"]["search_type"] != 0:  # (the KD-tree finder parks nothing: always 4)
        assert p["surv_slots"] == SLOT_WIDTHS[row["max_fixed"]], row["id"]
    elif p["split"]:
        assert p["surv_slots"] == 4


KITTI_ROW = dict(cfg="kitti", no_lone=0, max_fixed=512)


def test_max_fixed_edges():
    """SLOTS 4 / 8 at 512 / 513, split / fused at 1024 / 1025, the largest bound the fused kernel's LDS holds, 2047 / 2048"""
    assert plan(KITTI_ROW, max_fixed=512)["kernels"][1] == GN("4, 4, false, 4, 1, 1") and plan(KITTI_ROW, max_fixed=513)["kernels"][1] == GN("8, 4, false, 4, 1, 1")
    tp = dict(KITTI_ROW, no_lone=1)
    assert plan(tp, max_fixed=512)["kernels"][1] == GN("4, 4, false, 4, 4, 1") and plan(tp, max_fixed=513)["kernels"][1] == GN("8, 4, false, 3, 5, 1")
    assert (plan(tp, max_fixed=512)["five"], plan(tp, max_fixed=513)["five"]) == (0, 1)
    assert plan(KITTI_ROW, max_fixed=1024)["split"] == 1 and len(plan(KITTI_ROW, max_fixed=1024)["kernels"]) == 2
    fused = plan(KITTI_ROW, max_fixed=1025)
    assert fused["split"] == 0 and fused["kernels"] == [AK("256, false, -1, 4")]
    # a bound above the stride is the stride
    assert plan(KITTI_ROW, max_fixed=2000, stride=700)["max_fixed"] == 700
    at = plan(KITTI_ROW, max_fixed=FUSED_LIMIT)
    assert at["status"] == 0 and at["launches"][0]["lds"] == 160 * 1024
    for n in (FUSED_LIMIT + 1, 2047):
        over = plan(KITTI_ROW, max_fixed=n)
        assert (over["status"], over["kernels"]) == (_lib.ERR_UNSUPPORTED, []) and "does not fit the 160 KiB LDS" in over["message"]
    assert plan(KITTI_ROW, max_fixed=2048)["status"] == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("cus", [256, 304, 8])
def test_batch_edges_of_the_lone_instantiation(cus):
    at, above = plan(KITTI_ROW, batch=2 * cus, cus=cus), plan(KITTI_ROW, batch=2 * cus + 1, cus=cus)
    assert (at["lone"], above["lone"]) == (1, 0)
    assert at["kernels"][1] == GN("4, 4, false, 4, 1, 1") and above["kernels"][1] == GN("4, 4, false, 4, 4, 1")
    assert above["launches"][1]["grid_x"] == 2 * cus + 1
    assert plan(dict(KITTI_ROW, no_lone=1), batch=1, cus=cus)["lone"] == 0


def test_stamps_take_the_fused_kernel_unless_split_stamps_are_on():
    assert plan(KITTI_ROW, stamps=1)["kernels"] == [AK("256, false, -1, 4")]
    assert len(plan(KITTI_ROW, stamps=1, stamps_split=1)["kernels"]) == 2
