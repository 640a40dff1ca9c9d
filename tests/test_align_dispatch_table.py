"""The parity table of tests/test_align_dispatch_gpu.py names every kernel instantiation align_batch_launch can dispatch to (no GPU
needed): a new gn_kernel / align_kernel instantiation in the dispatch without a parity row fails here."""
import os
import re

from test_align_dispatch_gpu import DISPATCH

ALIGN_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "srrg2_proslam_amd", "csrc", "align.hip")


def dispatched_instantiations():
    src = open(ALIGN_HIP).read()
    start = src.index("int align_batch_launch(prs_context* ctx")
    end = src.index("static int split_rounds(prs_context* ctx, SplitJob* job, int rounds) {", start)
    found = set()
    for name, args in re.findall(r"\b(gn_kernel|align_kernel)<([^<>;]*)>", src[start:end]):
        found.add((name, re.sub(r"\s+", "", args)))
    return found


def table_instantiations():
    named = set()
    for row in DISPATCH:
        if row["gn"] is not None:
            named.add(("gn_kernel", row["gn"]))
        named.add(("align_kernel", row["search"]))
    return named


def test_dispatch_block_is_found_and_holds_every_family():
    found = dispatched_instantiations()
    assert sum(n == "gn_kernel" for n, _ in found) == 14
    assert sum(n == "align_kernel" for n, _ in found) == 8  # 3 patterns x 2 slot widths, the KD-tree, the fused kernel


def test_every_dispatched_instantiation_has_a_parity_row():
    missing = dispatched_instantiations() - table_instantiations()
    assert not missing, "instantiations without a row in DISPATCH: %s" % sorted(missing)


def test_every_parity_row_names_a_dispatched_instantiation():
    stale = table_instantiations() - dispatched_instantiations()
    assert not stale, "rows naming no instantiation of the dispatch: %s" % sorted(stale)


def test_row_ids_are_unique():
    ids = [r["id"] for r in DISPATCH]
    assert len(ids) == len(set(ids))
