"""The table of tests/test_bruteforce_dispatch_gpu.py names every kernel bruteforce_batch_launch can launch, tests/bruteforce_dispatch.py
restates the host's choice with the constants the source spells, and every row holds the content it claims (no GPU needed): a new
kernel in the launch block without a row, a stale row, a changed limit, or a row whose clouds hold no candidates, no pool conflicts, no
Lowe rejections or a candidate count off its capacity edge fails here.  Rows whose batch depends on the CU count are built for 256."""
import os
import re

import pytest

import bruteforce_dispatch as bd
from test_bruteforce_dispatch_gpu import DISPATCH, check_claims

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "srrg2_proslam_amd", "csrc", "bruteforce.hip")
MODES = {"kBfFused": bd.FUSED, "kBfDense": bd.DENSE, "kBfRegister": bd.REGISTER}


def _src():
    return open(SRC).read()


def launch_block():
    src = _src()
    start = src.index("int bruteforce_batch_launch(prs_context* ctx")
    return src[start:src.index("\n}\n", start)]


def launched():
    """the kernels the launch block names, as a kernel trace prints them"""
    block = launch_block()
    found = set()
    # launch_mode(std::integral_constant<int, MODE>{}, ..) instantiates bruteforce_kernel<KPT, MODE> for every KPT its lambda spells
    lam = block[block.index("auto launch_mode = [&]"):]
    lam = lam[:lam.index("};")]
    kpts = [int(k) for k in re.findall(r"bruteforce_kernel<(\d+), M>", lam)]
    for mode in re.findall(r"launch_mode\(std::integral_constant<int, (\w+)>\{\}", block):
        for k in kpts:
            found.add(bd.kernel_name(k, MODES[mode]))
    for args in re.findall(r"launch\(bruteforce_kernel<([^<>;]*)>", block):
        a = [x.strip() for x in args.split(",")]
        if a[1] == "M":
            continue
        found.add(bd.kernel_name(int(a[0]), MODES[a[1]], a[2] == "true", int(a[3]) if len(a) > 3 else bd.THREADS))
    for name in re.findall(r"hipLaunchKernelGGL\((bruteforce_\w+),", block):
        found.add("prs::%s(prs::BfArgs)" % name)
    return found


def table():
    return {k for r in DISPATCH for k in r["kernels"]}


def test_launch_block_is_found_and_names_fifteen_kernels():
    found = launched()
    assert len(found) == 15
    assert found == set(bd.all_kernels())


def test_every_launched_kernel_has_a_row():
    missing = launched() - table()
    assert not missing, "kernels without a row in DISPATCH: %s" % sorted(missing)


def test_every_row_names_a_launched_kernel():
    stale = table() - launched()
    assert not stale, "rows naming no kernel of the launch block: %s" % sorted(stale)
    assert all(r["kernels"] for r in DISPATCH)


def test_every_kernel_meets_conflicts_and_lowe_rejections():
    """each kernel is reached by at least one row that claims (and, below, proves) pool conflicts and Lowe rejections on both sides"""
    rich = {k for r in DISPATCH if r["claims"].get("conflicts") and r["claims"].get("lowe") for k in r["kernels"]}
    assert rich == set(bd.all_kernels())


def test_the_kept_kernel_trace_lists_every_kernel():
    """profiles/bruteforce_dispatch/kernel_stats.csv: the kernel trace of one run of the GPU module on an MI355X"""
    import csv
    path = os.path.join(os.path.dirname(os.path.dirname(SRC)), "..", "profiles", "bruteforce_dispatch", "kernel_stats.csv")
    with open(path, newline="") as f:
        traced = {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}
    assert all(traced.get(k, 0) > 0 for k in bd.all_kernels()), sorted(set(bd.all_kernels()) - set(traced))


def test_row_ids_are_unique():
    ids = [r["id"] for r in DISPATCH]
    assert len(ids) == len(set(ids))


def test_restated_constants_match_the_source():
    src, block = _src(), launch_block()
    assert re.search(r"constexpr int kBfThreads = %d;" % bd.THREADS, src)
    assert re.search(r"constexpr int kBfLevels\s*= %d;" % bd.LEVELS, src)
    assert "enum { kBfFused = %d, kBfDense = %d, kBfRegister = %d };" % (bd.FUSED, bd.DENSE, bd.REGISTER) in src
    assert re.search(r"constexpr int kMxSeg\s*= %d;" % bd.MX_SEG, src)
    assert "constexpr int kBfmPlaneRow = 64 + 16;" in src and bd.PLANE_ROW == 80
    assert re.search(r"constexpr int kBfmChunk\s*= %d;" % bd.MFMA_CHUNK, src)
    assert re.search(r"constexpr int kBfmWaveList = %d;" % bd.MFMA_WAVE_LIST, src)
    assert re.search(r"constexpr int kBfmFlushAt\s*= %d;" % bd.MFMA_FLUSH_AT, src)
    assert re.search(r"constexpr int kBfmThreads\s*= 512;", src) and re.search(r"constexpr int kBfmRowsWave = 64;", src)
    assert re.search(r"constexpr int kBfmRowsWg\s*= kBfmRowsWave \* \(kBfmThreads / 64\);", src) and bd.MFMA_ROWS_WG == 64 * (512 // 64)
    assert ("return 2u * 4u * (uint32_t) (chunk * kBfmPlaneRow) + 2u * (uint32_t) chunk * 4u + 2u * 16u * 4u + (uint32_t) (threads / 64) * kMxSeg * 16u;"
            in src)
    assert "kMxBytes = bf_mx_bytes(kBfThreads, 64), kMxBytesDual = bf_mx_bytes(512, 32);" in src
    assert "if (off > 160u * 1024u) {" in block and bd.LDS_LIMIT == 160 * 1024
    assert "off + bm_bytes + 4096u <= 160u * 1024u" in block
    assert "const uint32_t lds_limit_dual = 80u * 1024u - 512u;" in block and bd.LDS_LIMIT_DUAL == 80 * 1024 - 512
    assert "batch->fixed_stride > %d || batch->moving_stride > %d" % (bd.MAX_FIXED, bd.MAX_MOVING) in block
    assert "batch->batch * 2 <= cus && batch->moving_stride >= %d" % bd.SPLIT_MOVING in block
    assert ("matrix_when_full && batch->batch >= %d && batch->fixed_stride >= %d && batch->moving_stride >= %d"
            % (bd.FULL_BATCH, bd.FULL_FIXED, bd.FULL_MOVING)) in block
    assert "while (lim <= 257 && (float) lim < params->maximum_descriptor_distance) {" in block
    assert "a.nw  = lim > 0 ? (lim + 31) / 32 : 1;" in block
    assert "a.cap = batch->candidate_capacity > 0 ? batch->candidate_capacity : 16 * big;" in block
    assert "const int most = batch->moving_stride / 32;" in block
    for message in bd.REFUSALS.values():
        assert '"%s"' % message in block
    # the LDS carve: the six arrays of the registration state, in the order the restatement adds them up
    sizes = re.findall(r"a\.off_\w+\s*= off; off = bf_align16\(off \+ (.+?)\);", block)
    assert [re.sub(r"\(uint32_t\) |batch->", "", s) for s in sizes] == ["fixed_stride * 4", "moving_stride * 4", "fixed_stride", "moving_stride",
                                                                         "fixed_stride * 4", "(4 * kBfLevels + 8) * 4"]


def test_restated_dispatch_edges():
    d = bd.dispatch
    assert bd.MX_BYTES == 2 * 4 * 64 * 80 + 512 + 128 + 16 * 192 * 16 and bd.MX_BYTES_DUAL == 2 * 4 * 32 * 80 + 256 + 128 + 8 * 192 * 16
    assert [bd.limit_of(x) for x in (0.0, -1.0, float("nan"), 1.0, 31.5, 32.0, 255.5, 256.0, 256.5)] == [0, 0, 0, 1, 32, 32, 256, 256, 257]
    assert [d(1, 64, 64, x, 0, 0, 256)["nw"] for x in (0.0, 1.0, 32.0, 33.0, 64.0, 65.0, 256.0)] == [1, 1, 1, 2, 2, 3, 8]
    assert d(1, 8193, 8, 50.0, 0, 1, 256)["refused"] == "stride" and d(1, 8192, 65536, 50.0, 0, 1, 256)["refused"] == "stride"
    assert d(1, 64, 64, 256.5, 0, 1, 256)["refused"] == "threshold" and d(1, 8192, 30000, 50.0, 0, 1, 256)["refused"] == "lds"
    # the split shape: at most half as many pairs as CUs and a moving stride of 256
    assert d(128, 1024, 256, 50.0, 0, 0, 256)["chunks"] == 2 and d(129, 1024, 256, 50.0, 0, 0, 256)["chunks"] == 1
    assert d(4, 1024, 255, 50.0, 0, 0, 256)["chunks"] == 1 and d(4, 1024, 2600, 50.0, 0, 0, 256)["chunks"] == 64
    # the default's switch to the matrix cores, and to two workgroups per CU
    assert not d(31, 1024, 1024, 50.0, 0, 1, 256)["fused_matrix"] and d(32, 1024, 1024, 50.0, 0, 1, 256)["fused_matrix"]
    assert not d(256, 1024, 1024, 50.0, 0, 1, 256)["dual"] and d(257, 1024, 1024, 50.0, 0, 1, 256)["dual"]
    assert d(600, 1024, 1024, 50.0, 0, 1, 256)["grid"] == 512 and d(600, 1024, 1024, 50.0, 0, 1, 256, {"PRS_BF_TWO_WORKGROUPS": "0"})["grid"] == 256
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
