"""The parity table of tests/test_stereo_dispatch_gpu.py names every kernel instantiation the stereo matcher can dispatch to, and
tests/stereo_dispatch.py restates the host's limits and LDS layouts as the source spells them (no GPU needed): a new launch5 /
launch_variant instantiation without a parity row, a stale row, or a changed limit or carve fails here."""
import os
import re

import pytest

import stereo_dispatch as sd
from test_stereo_dispatch_gpu import DISPATCH, STANDALONE

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "srrg2_proslam_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _block(src, start, end):
    i = src.index(start)
    return src[i:src.index(end, i)]


def v5_block():
    return _block(_src("stereo_match_v5.hip"), "int stereo_match_v5_launch(prs_context* ctx", "\n}\n")


def first_gen_block():
    return _block(_src("stereo_match.hip"), "int stereo_match_batch_launch(prs_context* ctx", "\n}\n")


def dispatched_instantiations():
    v5 = _src("stereo_match_v5.hip")
    body = _block(v5, "hipError_t launch5(const Args5& a", "\n}\n")
    combos = {re.sub(r"\s+", "", c) for c in re.findall(r"stereo_match5_kernel<KPT,([^<>;]*)>", body)}
    found = set()
    for kpt in re.findall(r"\blaunch5<(\d+)>", v5_block()):
        for c in combos:
            found.add(("stereo_match5_kernel", "%s,%s" % (kpt, c)))
    for args in re.findall(r"\blaunch_variant<([^<>;]*)>", first_gen_block()):
        found.add(("stereo_match_kernel", re.sub(r"\s+", "", args)))
    for name in re.findall(r"hipLaunchKernelGGL\((triangulate_kernel)\b", _src("stereo_match.hip")):
        found.add((name, ""))
    return found


def table_instantiations():
    return {(r["kernel"], r["args"]) for r in DISPATCH} | set(STANDALONE)


def test_dispatch_blocks_are_found_and_hold_every_family():
    found = dispatched_instantiations()
    assert sum(n == "stereo_match5_kernel" for n, _ in found) == 8  # KPT 1 / 2 x MULTI x EPI
    assert sum(n == "stereo_match_kernel" for n, _ in found) == 6   # staged KPT 1 / 2, unstaged KPT 1 / 2 / 4 / 8
    assert ("triangulate_kernel", "") in found
    assert len(found) == 15


def test_every_dispatched_instantiation_has_a_parity_row():
    missing = dispatched_instantiations() - table_instantiations()
    assert not missing, "instantiations without a row in DISPATCH: %s" % sorted(missing)


def test_every_parity_row_names_a_dispatched_instantiation():
    stale = table_instantiations() - dispatched_instantiations()
    assert not stale, "rows naming no instantiation of the dispatch: %s" % sorted(stale)


def test_row_ids_are_unique():
    ids = [r["id"] for r in DISPATCH]
    assert len(ids) == len(set(ids))


def test_every_row_is_chosen_by_its_knobs():
    for r in DISPATCH:
        d = sd.dispatch(r["stride"], 376, r["thickness"], 100.0, r["epi"], r.get("v3", 0), r.get("unstaged", 0))
        assert (d["kernel"], d["args"]) == (r["kernel"], r["args"]), r["id"]
        assert max(r["n"]) == r["stride"] and len(set(r["n"])) == len(r["n"]), r["id"]  # a full frame, distinct counts


def test_restated_limits_match_the_source():
    v5, g = v5_block(), first_gen_block()
    v5_all = _src("stereo_match_v5.hip")
    assert re.search(r"constexpr int kT\s*=\s*%d;" % sd.KT, v5_all)
    assert re.search(r"constexpr int kStereoThreads\s*=\s*%d;" % sd.KT, _src("stereo_match.hip"))
    assert "stride > 2 * kT" in v5 and sd.V5_MAX_STRIDE == 2 * sd.KT
    assert "if (cap > %du) {" % sd.V5_CAP_MAX in v5
    assert "if (off > 160u * 1024u) {" in v5 and sd.LDS_LIMIT == 160 * 1024
    assert "a.pool_cap = (int) (((160u * 1024u - off) / 4u) & ~3u);" in v5
    assert "a.pool_cap > %d ? %d : (a.pool_cap < %d ? 0 : a.pool_cap)" % (sd.POOL_MAX, sd.POOL_MAX, sd.POOL_MIN) in v5
    assert "if (a.best_lim > %d) {" % sd.V5_BEST_LIM_MAX in v5
    assert "ctx_force_unstaged(ctx) || ctx_matcher_v3(ctx)" in v5
    assert "const uint32_t cap = ((uint32_t) stride + 3u * (uint32_t) (rows < stride ? rows : stride) + 3u) & ~3u;" in v5
    assert "stride <= kT ? launch5<1>(a, lds, stream) : launch5<2>(a, lds, stream)" in v5
    assert "stride <= 0 || stride > %d || params->image_rows <= 0 || params->image_rows > %d" % (sd.MAX_STRIDE, sd.MAX_ROWS) in g
    assert "epipolar_line_thickness_pixels > %d" % sd.MAX_THICKNESS in g
    assert "const size_t lds_limit = 160 * 1024;" in g
    assert "stride <= 1024 ? 1 : (stride <= 2048 ? 2 : (stride <= 4096 ? 4 : 8))" in g
    assert "if (lds > lds_limit || kpt > 2 || ctx_force_unstaged(ctx)) {" in g
    assert "const bool multi = a.p.epipolar_line_thickness_pixels > 0;" in _block(v5_all, "hipError_t launch5(const Args5& a", "\n}\n")
    # fill_accept_table: the loop bounds the restatement copies
    t = _block(_src("stereo_match.hip"), "void fill_accept_table(", "\n}\n")
    assert "while (lim <= 256 && (float) lim < max_dist) {" in t and "for (int s = 0; s <= 257; ++s) {" in t
    assert "bmax[s] = (int16_t) (s == 0 ? -1 : bm);" in t


def _c_to_py(expr):
    """one carve size expression of the source as Python: casts and unsigned suffixes dropped, `stage ? x : 0` as a conditional"""
    expr = re.sub(r"\((?:uint32_t|int|size_t)\)\s*", "", expr)
    expr = re.sub(r"\b(\d+)u\b", r"\1", expr)
    expr = re.sub(r"\bs\.|\ba\.", "", expr)
    expr = re.sub(r"\(?stage \? ([^:]+?) : 0\)?", r"((\1) if stage else 0)", expr)
    return expr.replace("/", "//")


def _v5_carve_from_source(stride, rows):
    v5 = v5_block()
    sizes = re.findall(r"a\.off_\w+\s*= off; off = up16\(off \+ (.+?)\);", v5)
    assert len(sizes) == 13
    cap = sd.v5_layout(stride, rows)["cap"]
    env = dict(stride=stride, rows=rows, cap=cap, nwords=(cap + 31) // 32, rows2=rows + 2, PRS_DESC_BYTES=sd.DESC_BYTES)
    off = 0
    for e in sizes:
        off = (off + eval(_c_to_py(e), {}, env) + 15) & ~15
    return off


def _first_gen_carve_from_source(stride, rows, stage):
    g = first_gen_block()
    lam = _block(g, "auto carve = [&](bool stage, StereoArgs& s) -> size_t {", "return off;")
    dbytes = re.search(r"const uint32_t dbytes = (.+?);", lam).group(1)
    sizes = re.findall(r"s\.off_\w+\s*= off; off = align_up\(off \+ (.+?), 16\);", lam)
    assert len(sizes) == 11
    rows1 = rows + 1
    env = dict(stride=stride, rows=rows, rows1=rows1, sort_cap=max(stride, rows1), nwords=(stride + 31) // 32, stage=stage,
               PRS_DESC_BYTES=sd.DESC_BYTES)
    env["dbytes"] = eval(_c_to_py(dbytes), {}, env)
    off = 0
    for e in sizes:
        off = (off + eval(_c_to_py(e), {}, env) + 15) // 16 * 16
    return off


@pytest.mark.parametrize("stride,rows", [(1, 1), (64, 4096), (1000, 2094), (1000, 2095), (1024, 376), (2000, 376), (2048, 480), (2048, 489),
                                         (2048, 490), (2048, 493), (8192, 4096), (4097, 17)])
def test_restated_layouts_match_the_source_carves(stride, rows):
    lay = sd.v5_layout(stride, rows)
    if lay["why"] != "cap":
        before_pool = lay["off_pool"] if lay["fits"] else lay["lds"]
        assert _v5_carve_from_source(stride, rows) == before_pool
    for stage in (True, False):
        assert _first_gen_carve_from_source(stride, rows, stage) == sd.first_gen_carve(stride, rows, stage)


def test_layout_edges():
    """the shapes at which the pool and the v5 layout change; the 13-bit cap never refuses a layout that would fit"""
    assert sd.v5_layout(2048, 489)["pool_cap"] == 64
    assert sd.v5_layout(2048, 490)["pool_cap"] == 0 and sd.v5_layout(2048, 492)["fits"]
    assert sd.v5_layout(2048, 493)["why"] == "lds"
    assert sd.v5_layout(1000, 2094)["pool_cap"] == 72 and sd.v5_layout(1000, 2095)["pool_cap"] == 0
    assert sd.v5_layout(2000, 376)["pool_cap"] == 3072
    assert sd.v5_layout(2048, 480)["pool_cap"] == 248
    assert sd.v5_layout(1024, 376)["pool_cap"] == sd.POOL_MAX
    assert sd.v5_layout(2047, 2047)["cap"] == sd.V5_CAP_MAX and sd.v5_layout(2048, 2048)["why"] == "cap"
    for stride in range(1, 2049, 31):
        for rows in range(stride - 40, stride + 3000, 97):
            if rows >= 1 and (stride + 3 * min(rows, stride) + 3) & ~3 > sd.V5_CAP_MAX:
                lay = sd.v5_layout(stride, rows)
                assert lay["why"] == "cap"
                # the same layout without the cap check would not fit either
                assert _v5_carve_from_source(stride, rows) > sd.LDS_LIMIT


def test_acceptance_table_edges():
    assert [sd.fill_accept_table(x, 0.5)[0] for x in (255.0, 255.5, 256.0, 256.5)] == [255, 256, 256, 257]
    lim, bmax = sd.fill_accept_table(100.0, 1.5)
    assert bmax[0] == -1 and bmax[1] == 1 and bmax[257] == 256
    _, bmax = sd.fill_accept_table(100.0, 0.8)
    assert bmax[10] == 7
