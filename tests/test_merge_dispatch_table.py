"""The parity table of tests/test_merge_dispatch_gpu.py names every kernel merge_batch_launch can launch (no GPU needed): a new
merge_kernel instantiation or smoother kernel in the dispatch without a row fails here, and so does a row that names none."""
import os
import re

from test_merge_dispatch_gpu import DISPATCH

MAPPING_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "srrg2_proslam_amd", "csrc", "mapping.hip")


def dispatch_block():
    src = open(MAPPING_HIP).read()
    start = src.index("int merge_batch_launch(prs_context* ctx")
    end = src.index("// pose_out = prediction * X^-1", start)
    return src[start:end]


def dispatched():
    block = dispatch_block()
    found = {("merge_kernel", re.sub(r"\s+", "", args)) for args in re.findall(r"\bmerge_kernel<([^<>;]*)>", block)}
    found |= {(name, "") for name in re.findall(r"hipLaunchKernelGGL\(\s*(\w+)\s*,", block) if name != "kernel"}
    return found


def table():
    named = set()
    for row in DISPATCH:
        named |= {("merge_kernel", args) for args in row["merge"]}
        named |= {(name, "") for name in row["smoother"]}
    return named


def test_dispatch_block_is_found_and_holds_every_kernel():
    found = dispatched()
    assert sum(n == "merge_kernel" for n, _ in found) == 7
    assert {n for n, _ in found if n != "merge_kernel"} == {"smoother_kernel", "smoother_tail_kernel"}


def test_every_dispatched_kernel_has_a_row():
    missing = dispatched() - table()
    assert not missing, "kernels without a row in DISPATCH: %s" % sorted(missing)


def test_every_row_names_a_dispatched_kernel():
    stale = table() - dispatched()
    assert not stale, "rows naming no kernel of the dispatch: %s" % sorted(stale)
    assert all(row["merge"] for row in DISPATCH)


def test_row_ids_are_unique():
    ids = [r["id"] for r in DISPATCH]
    assert len(ids) == len(set(ids))
