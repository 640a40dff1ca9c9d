"""The launch-size rule in the dispatch plans (prs::Plan::add, csrc/prs_host.h): every grid a plan holds has passed prs_launch_fits with
its launch's block, so a batch of one workgroup a frame, pair or map too many is refused by the plan -- PRS_ERR_UNSUPPORTED, no launch,
the entry point's name and one text -- and the launcher that takes the plan enqueues nothing.  Every shape here has a grid that IS the
batch (the persistent grids, which the CU count caps, never reach the limit).  Plans follow no batch pointer: no GPU, no memory."""
import pytest

import bruteforce_dispatch as bd
from srrg2_proslam_amd import _lib
from test_align_dispatch_table import KITTI_ROW, plan as align_plan
from test_bruteforce_dispatch_table import plan as bruteforce_plan
from test_merge_dispatch_gpu import DISPATCH as MERGE_ROWS, row_kernels as merge_row_kernels
from test_merge_dispatch_table import plan as merge_plan
from test_stereo_dispatch_table import plan as stereo_plan

TEXT = ": more work-items than one launch holds"


@pytest.fixture(scope="module")
def fits():
    return _lib.load().prs_launch_fits


def first_refused(fits, block):
    """the smallest batch of one workgroup each that prs_launch_fits refuses for this block, by bisection"""
    lo, hi = 1, 1 << 33  # fits, does not
    assert fits(lo, block) == 1 and fits(hi, block) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid, block) == 1 else (lo, mid)
    return hi


def stereo(batch):  # the first generation's unstaged kernel: one workgroup a frame
    return stereo_plan(1024, 376, 1, 100.0, 0, v3=1, unstaged=1, batch=batch)


def align_fused(batch):  # the fused kernel: one workgroup a frame
    return align_plan(dict(KITTI_ROW, fused=1), batch=batch)


def bruteforce(batch):  # forced matrix cores without the fused shape: the dense launch has the pairs in y, the registration in x
    return bruteforce_plan(batch, 512, 512, 60.0, 0, bd.MATRIX, 256, {"PRS_BF_GLOBAL_STATE": "1"})


def merge(batch):  # a one-kernel merger: one workgroup a map
    row = next(r for r in MERGE_ROWS if len(merge_row_kernels(r)) == 1)
    return merge_plan(row, batch=batch)


FAMILIES = [("prs_stereo_match_batch", stereo), ("prs_align_batch_run", align_fused), ("prs_bruteforce_match", bruteforce),
            ("prs_merge_batch_run", merge)]


@pytest.mark.parametrize("entry,plan", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_the_last_batch_that_fits_and_the_first_that_does_not(fits, entry, plan):
    """the edge follows from prs_launch_fits and the blocks of the family's per-item launches: 2^24 for the aligner's fused kernel and
    the merger (256 threads), 2^22 for the first-generation stereo matcher and the brute-force registration (1024 threads)"""
    small = plan(6)
    assert small["status"] == 0 and small["launches"], small
    per_item = [i for i, l in enumerate(small["launches"]) if 6 in (l["grid_x"], l["grid_y"])]
    assert per_item, small
    # a batch in y is a grid dimension of its own, of one thread a workgroup
    edge = min(first_refused(fits, small["launches"][i]["block"] if small["launches"][i]["grid_x"] == 6 else 1) for i in per_item)
    blocks = {small["launches"][i]["block"] for i in per_item if small["launches"][i]["grid_x"] == 6}
    assert edge == (1 << 32) // max(blocks) and (max(blocks) != 256 or edge == 1 << 24), (edge, blocks)
    at = plan(edge - 1)
    assert at["status"] == 0 and at["message"] is None and at["kernels"] == small["kernels"], at
    for i in per_item:
        l, s = at["launches"][i], small["launches"][i]
        assert (l["grid_x"] if s["grid_x"] == 6 else l["grid_y"]) == edge - 1 and l["block"] == s["block"] and l["lds"] == s["lds"], l
    over = plan(edge)
    assert (over["status"], over["message"], over["launches"], over["kernels"]) == (_lib.ERR_UNSUPPORTED, entry + TEXT, [], []), over


def test_the_split_aligner_is_refused_where_its_widest_workgroup_is(fits):
    """search launch: 512 threads a frame, Gauss-Newton launch: 128; a batch is planned when BOTH fit"""
    small = align_plan(KITTI_ROW)
    assert small["split"] and [l["block"] for l in small["launches"]] == [512, 128]
    edge_search, edge_gn = first_refused(fits, 512), first_refused(fits, 128)
    assert edge_search < edge_gn
    for batch in (edge_search - 1, edge_search, edge_gn - 1, edge_gn):
        p, ok = align_plan(KITTI_ROW, batch=batch), fits(batch, 512) == 1 and fits(batch, 128) == 1
        if ok:
            assert p["status"] == 0 and [(l["grid_x"], l["grid_y"], l["block"]) for l in p["launches"]] == [(batch, 1, 512), (batch, 1, 128)], p
        else:
            assert (p["status"], p["message"], p["launches"]) == (_lib.ERR_UNSUPPORTED, "prs_align_batch_run" + TEXT, []), p
    assert align_plan(KITTI_ROW, batch=edge_search - 1)["status"] == 0 and align_plan(KITTI_ROW, batch=edge_search)["status"] != 0


def test_a_refusal_for_another_reason_keeps_its_text():
    """the limit is the last thing a plan looks at: a shape it refuses anyway says why"""
    p = stereo_plan(9000, 376, 1, 100.0, 0, batch=1 << 24)
    assert p["status"] == _lib.ERR_UNSUPPORTED and p["message"].startswith("prs_stereo_match_batch: stride must be")
