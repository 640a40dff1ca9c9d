"""The table of tests/test_bruteforce_dispatch_gpu.py names every kernel the brute-force matcher can launch, tests/bruteforce_dispatch.py
restates the host's choice exactly as the library plans it, and every row holds the content it claims (no GPU needed): a new kernel in
the library's variant table without a row, a stale row, a limit or choice that the restatement and prs_bruteforce_plan disagree on, or a
row whose clouds hold no candidates, no pool conflicts, no Lowe rejections or a candidate count off its capacity edge fails here.  Rows
whose batch depends on the CU count are built for 256."""
import csv
import itertools
import os

import pytest

import bruteforce_dispatch as bd
from srrg2_proslam_amd import _lib, ops
from test_bruteforce_dispatch_gpu import DISPATCH, check_claims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO = "PRS_BF_TWO_WORKGROUPS"


def enumerated():
    return ops.dispatch_kernel_names(_lib.DISPATCH_BRUTEFORCE)


def table():
    return {k for r in DISPATCH for k in r["kernels"]}


def plan(batch, fixed_stride, moving_stride, max_dist, candidate_capacity, mode, cus, env=None):
    """prs_bruteforce_plan for the arguments of bd.dispatch"""
    env = env or {}
    e = ops.dispatch_env(cus=cus, bf_mfma=mode, bf_global_state="PRS_BF_GLOBAL_STATE" in env,
                         bf_two_workgroups=(1 if env[TWO][:1] == "1" else 0) if TWO in env else -1)
    b = _lib.BruteforceBatch(batch=batch, fixed_stride=fixed_stride, moving_stride=moving_stride, candidate_capacity=candidate_capacity)
    return ops.bruteforce_plan(ops.bruteforce_params(max_dist), b, e)


def check_against_plan(*args):
    """the restatement and the library's plan, field by field"""
    d, p = bd.dispatch(*args), plan(*args)
    batch, fs = args[0], args[1]
    if d["refused"]:
        assert (p["status"], p["message"], p["kernels"]) == (bd.ERR_UNSUPPORTED, bd.REFUSALS[d["refused"]], []), args
        return
    assert p["status"] == 0 and p["message"] is None and p["kernels"] == d["kernels"], (args, d, p)
    if not d["kernels"]:
        return
    for k in ("lim", "nw", "cap", "grid", "chunks", "bm_fits", "lvl_cap", "fused_matrix", "dual", "mfma", "lds"):
        assert p[k] == d[k], (k, args, d, p)
    threads = 512 if d["dual"] else bd.THREADS
    if d["chunks"] > 1:
        dense = dict(grid_x=-(-fs // bd.MFMA_ROWS_WG), grid_y=batch, block=512, lds=0) if d["mfma"] else dict(grid_x=d["chunks"], grid_y=batch,
                                                                                                         block=bd.THREADS, lds=d["lds"])
        want = [dense, dict(grid_x=batch, grid_y=1, block=bd.THREADS, lds=d["lds"])]
    else:
        want = [dict(grid_x=d["grid"], grid_y=1, block=threads, lds=d["lds"])]
    assert [{k: v for k, v in l.items() if k != "kernel"} for l in p["launches"]] == want, (args, p)
    # the carve in front of the bitmaps: six 16-byte aligned arrays in this order
    up16 = lambda v: (v + 15) & ~15  # noqa: E731
    offs = list(itertools.accumulate([fs * 4, args[2] * 4, fs, args[2], fs * 4, (4 * bd.LEVELS + 8) * 4], lambda off, size: up16(off) + size, initial=0))
    assert [p[k] for k in ("off_cnt_f", "off_cnt_m", "off_reg_f", "off_reg_m", "off_acc", "off_hist")] == [up16(o) for o in offs[:6]], args
    assert p["off_bm"] == (up16(offs[6]) if d["bm_fits"] else 0xffffffff - (1 << 32)) and p["off_lvl"] == p["off_mx"], args


def test_variant_table_names_fifteen_kernels():
    found = enumerated()
    assert len(found) == len(set(found)) == 15
    assert set(found) == set(bd.all_kernels())


def test_every_launched_kernel_has_a_row():
    missing = set(enumerated()) - table()
    assert not missing, "kernels without a row in DISPATCH: %s" % sorted(missing)


def test_every_row_names_a_launched_kernel():
    stale = table() - set(enumerated())
    assert not stale, "rows naming no kernel of the variant table: %s" % sorted(stale)
    assert all(r["kernels"] for r in DISPATCH)


def test_every_kernel_meets_conflicts_and_lowe_rejections():
    """each kernel is reached by at least one row that claims (and, below, proves) pool conflicts and Lowe rejections on both sides"""
    rich = {k for r in DISPATCH if r["claims"].get("conflicts") and r["claims"].get("lowe") for k in r["kernels"]}
    assert rich == set(enumerated())


def test_the_kept_kernel_trace_lists_every_kernel():
    """profiles/bruteforce_dispatch/kernel_stats.csv: the kernel trace of one run of the GPU module on an MI355X"""
    with open(os.path.join(ROOT, "profiles", "bruteforce_dispatch", "kernel_stats.csv"), newline="") as f:
        traced = {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}
    assert all(traced.get(k, 0) > 0 for k in enumerated()), sorted(set(enumerated()) - set(traced))


def test_row_ids_are_unique():
    ids = [r["id"] for r in DISPATCH]
    assert len(ids) == len(set(ids))


BATCHES = (0, 1, 2, 4, 31, 32, 33, 127, 128, 129, 255, 256, 257, 600)
FIXED = (0, 1, 33, 255, 256, 257, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)
MOVING = (0, 1, 63, 64, 65, 200, 255, 256, 257, 1024, 2600, 8192, 16000, 30000, 65535, 65536)
THRESHOLDS = (0.0, -1.0, 1.0, 31.5, 32.0, 33.0, 50.0, 64.0, 65.0, 255.5, 256.0, 256.5, float("nan"))
ENVS = ({}, {"PRS_BF_GLOBAL_STATE": "1"}, {TWO: "0"}, {TWO: "1"}, {"PRS_BF_GLOBAL_STATE": "1", TWO: "1"})


def test_restatement_equals_the_library_plan_over_a_sweep():
    """every limit the restatement holds, at its edges and their neighbours (about 60 000 combinations)"""
    n = 0
    for batch, fs, ms, mode, env in itertools.product(BATCHES, FIXED, MOVING, (bd.POPCOUNT, bd.MATRIX_WHEN_FULL, bd.MATRIX), ENVS):
        check_against_plan(batch, fs, ms, 50.0, 0, mode, 256, env)
        n += 1
    # thresholds (lim, nw, what fits beside wider bitmaps), the capacity rule and another CU count: on the shapes around each switch
    for batch, fs, ms, x, cap, mode, cus in itertools.product((1, 32, 128, 257), (64, 1024, 4096), (64, 256, 1024, 8192), THRESHOLDS, (0, 9),
                                                           (bd.POPCOUNT, bd.MATRIX_WHEN_FULL, bd.MATRIX), (256, 304, 64)):
        check_against_plan(batch, fs, ms, x, cap, mode, cus, {})
        n += 1
    assert n > 50000


def test_restated_dispatch_edges():
    def d(*args):
        check_against_plan(*args)
        return bd.dispatch(*args)
    assert bd.MX_BYTES == 2 * 4 * 64 * 80 + 512 + 128 + 16 * 192 * 16 and bd.MX_BYTES_DUAL == 2 * 4 * 32 * 80 + 256 + 128 + 8 * 192 * 16
    limits = (0.0, -1.0, float("nan"), 1.0, 31.5, 32.0, 255.5, 256.0)
    assert [bd.limit_of(x) for x in limits + (256.5,)] == [0, 0, 0, 1, 32, 32, 256, 256, 257]
    assert [plan(1, 64, 64, x, 0, 0, 256)["lim"] for x in limits] == [0, 0, 0, 1, 32, 32, 256, 256]
    assert [d(1, 64, 64, x, 0, 0, 256)["nw"] for x in (0.0, 1.0, 32.0, 33.0, 64.0, 65.0, 256.0)] == [1, 1, 1, 2, 2, 3, 8]
    assert d(1, 8193, 8, 50.0, 0, 1, 256)["refused"] == "stride" and d(1, 8192, 65536, 50.0, 0, 1, 256)["refused"] == "stride"
    assert d(1, 64, 64, 256.5, 0, 1, 256)["refused"] == "threshold" and d(1, 8192, 30000, 50.0, 0, 1, 256)["refused"] == "lds"
    # the split shape: at most half as many pairs as CUs and a moving stride of 256
    assert d(128, 1024, 256, 50.0, 0, 0, 256)["chunks"] == 2 and d(129, 1024, 256, 50.0, 0, 0, 256)["chunks"] == 1
    assert d(4, 1024, 255, 50.0, 0, 0, 256)["chunks"] == 1 and d(4, 1024, 2600, 50.0, 0, 0, 256)["chunks"] == 64
    # the default's switch to the matrix cores, and to two workgroups per CU
    assert not d(31, 1024, 1024, 50.0, 0, 1, 256)["fused_matrix"] and d(32, 1024, 1024, 50.0, 0, 1, 256)["fused_matrix"]
    assert not d(256, 1024, 1024, 50.0, 0, 1, 256)["dual"] and d(257, 1024, 1024, 50.0, 0, 1, 256)["dual"]
    assert d(600, 1024, 1024, 50.0, 0, 1, 256)["grid"] == 512 and d(600, 1024, 1024, 50.0, 0, 1, 256, {TWO: "0"})["grid"] == 256
    assert d(4, 1024, 1024, 50.0, 0, 2, 256)["mfma"] and d(4, 1024, 200, 50.0, 0, 2, 256)["fused_matrix"]
    assert not d(2, 1024, 1024, 50.0, 0, 0, 256, {"PRS_BF_GLOBAL_STATE": "1"})["bm_fits"]
    assert d(2, 4096, 8192, 32.0, 0, 0, 256)["lvl_cap"] == 8184 and not d(2, 4096, 8192, 33.0, 0, 0, 256)["bm_fits"]
    assert d(1, 33, 33, 50.0, 0, 0, 256)["cap"] == 16 * 33 and d(1, 33, 70, 50.0, 9, 0, 256)["cap"] == 9


@pytest.mark.parametrize("r", DISPATCH, ids=[r["id"] for r in DISPATCH])
def test_row_holds_what_it_claims(oracle, r):
    cus = 256
    case = r["make"](cus)
    d = check_claims(r, case, cus, oracle)
    for max_dist, _ in case.launches:
        assert case.dispatch(cus, max_dist)["kernels"] == r["kernels"] == d["kernels"]
        assert plan(len(case.pairs), case.fs, case.ms, max_dist, case.cap, case.mode, cus, case.env)["kernels"] == r["kernels"]
