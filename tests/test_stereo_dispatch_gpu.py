"""Every instantiation the stereo matcher's dispatch can reach, against the C oracle, and the kernels' capacity and data-path edges.

stereo_plan (csrc/stereo_match.hip, with the v5 layout of csrc/stereo_match_v5.hip) chooses among
stereo_match5_kernel<KPT, MULTI, EPI> (8), stereo_match_kernel<KPT, STAGE> (6) and, for prs_triangulate, triangulate_kernel.
DISPATCH names one row per instantiation with the knobs that select it; tests/stereo_dispatch.py restates the host's choice and
every row asserts that its knobs pick its variant; tests/test_stereo_dispatch_table.py checks (without a GPU) that the library's
variant tables name no instantiation without a row and that the restatement equals the library's plan.  Every frame of every batch is compared with the oracle: correspondences including
their order and response bits, status / warning bits and, with the fused epilogue, n_fixed and the bits of fixed_uvuv, fixed_desc
and fixed_xyz (validity included).  The edge rows then pin the shape limits, the layout fallbacks, the acceptance table's
extremes, the candidate pool (windows of four / five, pool partly used, pool exhausted and the replay sweep, pool_cap 64 / 0), the
two scan branches, the sentinel padding, the coordinate domain and the persistent grid; each asserts from the restatement that it
reaches its path.  Last, the epilogue's triangulated points against a float64 restatement."""
import numpy as np
import pytest

import stereo_dispatch as sd
import stereo_ref as sr
from helpers import corr_equal, oracle_stereo_params, oracle_tri_params
from srrg2_proslam_amd import configs, ops, synthetic as syn

pytestmark = pytest.mark.gpu

KITTI = configs.get("kitti")
M_KITTI = dict(KITTI["stereo_matcher"])
# crafted windows: an accepted best at the acceptance table's edge needs a ratio whose bmax[second] is below second
M_EDGE = {"maximum_descriptor_distance": 100.0, "maximum_distance_ratio_to_second_best": 0.8, "minimum_matching_ratio": 0.1,
          "maximum_disparity_pixels": 20, "epipolar_line_thickness_pixels": 0}

# One row per instantiation.  kernel / args as the dispatch spells them (whitespace removed); v3: PRS_MATCHER_V3=1, unstaged:
# PRS_FORCE_UNSTAGED=1; n: keypoints of each frame of the batch (left, right), stride: the batch's keypoint stride.
DISPATCH = [
    dict(id="v5_k1_single", stride=1024, n=[1024, 700, 1, 333], thickness=0, epi=0, kernel="stereo_match5_kernel", args="1,false,false"),
    dict(id="v5_k1_single_epi", stride=1000, n=[1000, 999, 64, 500], thickness=0, epi=1, kernel="stereo_match5_kernel", args="1,false,true"),
    dict(id="v5_k1_multi", stride=777, n=[777, 400, 2, 650], thickness=1, epi=0, kernel="stereo_match5_kernel", args="1,true,false"),
    dict(id="v5_k1_multi_epi", stride=1024, n=[1024, 1000, 513, 7], thickness=2, epi=1, kernel="stereo_match5_kernel", args="1,true,true"),
    dict(id="v5_k2_single", stride=2048, n=[2048, 1025, 1500, 90], thickness=0, epi=0, kernel="stereo_match5_kernel", args="2,false,false"),
    dict(id="v5_k2_single_epi", stride=2000, n=[2000, 1777, 1024, 300], thickness=0, epi=1, kernel="stereo_match5_kernel", args="2,false,true"),
    dict(id="v5_k2_multi", stride=1025, n=[1025, 1024, 600, 1], thickness=1, epi=0, kernel="stereo_match5_kernel", args="2,true,false"),
    dict(id="v5_k2_multi_epi", stride=2048, n=[2048, 2000, 1100, 64], thickness=2, epi=1, kernel="stereo_match5_kernel", args="2,true,true"),
    dict(id="g_k1_staged", stride=1024, n=[1024, 800, 3, 512], thickness=1, epi=1, v3=1, kernel="stereo_match_kernel", args="1,true"),
    dict(id="g_k1_staged_plain", stride=900, n=[900, 450, 20, 899], thickness=0, epi=0, v3=1, kernel="stereo_match_kernel", args="1,true"),
    dict(id="g_k2_staged", stride=2048, n=[2048, 1500, 1025, 40], thickness=0, epi=1, v3=1, kernel="stereo_match_kernel", args="2,true"),
    dict(id="g_k1_unstaged", stride=600, n=[600, 599, 1, 300], thickness=2, epi=1, unstaged=1, kernel="stereo_match_kernel", args="1,false"),
    dict(id="g_k2_unstaged", stride=1800, n=[1800, 1200, 1100, 5], thickness=0, epi=0, unstaged=1, kernel="stereo_match_kernel", args="2,false"),
    dict(id="g_k2_unstaged_epi", stride=2048, n=[2048, 1300, 77, 1025], thickness=1, epi=1, unstaged=1, kernel="stereo_match_kernel", args="2,false"),
    dict(id="g_k4", stride=4096, n=[4096, 3000, 2049, 100], thickness=1, epi=1, kernel="stereo_match_kernel", args="4,false"),
    dict(id="g_k8", stride=8192, n=[8192, 5000, 4097, 1], thickness=0, epi=0, kernel="stereo_match_kernel", args="8,false"),
    dict(id="g_k8_epi", stride=6000, n=[6000, 4500, 300, 5999], thickness=1, epi=1, kernel="stereo_match_kernel", args="8,false"),
]
# instantiations reached outside the batched matcher (the test that reaches each)
STANDALONE = {("triangulate_kernel", ""): "test_standalone_triangulator_vs_float64"}

U = 2.0 ** -24  # unit roundoff of float32


@pytest.fixture
def make_ctx(monkeypatch):
    made = []

    def make(v3=0, unstaged=0):
        """a fresh context: the knobs are read when it is created"""
        for name, on in (("PRS_MATCHER_V3", v3), ("PRS_FORCE_UNSTAGED", unstaged)):
            if on:
                monkeypatch.setenv(name, "1")
            else:
                monkeypatch.delenv(name, raising=False)
        ctx = ops.Context(0)
        made.append(ctx)
        return ctx

    yield make
    for c in made:
        c.close()


def _tri(min_disp=None):
    tp = ops.triangulator_params(KITTI)
    if min_disp is not None:
        tp.minimum_disparity_pixels = min_disp
    return tp


def _expect(stride, rows, m, epi, v3=0, unstaged=0):
    return sd.dispatch(stride, rows, m["epipolar_line_thickness_pixels"], m["maximum_descriptor_distance"], epi, v3, unstaged)


def _assert_variant(d, kernel, args):
    assert d["refused"] is None and (d["kernel"], d["args"]) == (kernel, args), d


def run_batch(ctx, m, rows, data, stride, epi, tp=None, expect=None):
    """expect: (kernel, args) the library's plan for these inputs on this context must name (host only), before anything runs"""
    import torch
    frames = ops.StereoFrames(0, len(data), stride, epilogue=bool(epi))
    for b, fr in enumerate(data):
        frames.upload(b, fr["uv_left"], fr["desc_left"], fr["uv_right"], fr["desc_right"])
    params, tri = ops.stereo_params(m, rows), (tp or _tri()) if epi else None
    if expect is not None:
        assert ops.stereo_plan(params, frames.descriptor(tri), ops.dispatch_env(ctx))["kernels"] == [sd.trace_name(*expect)]
    ops.stereo_match_batch(ctx, params, frames, tri)
    torch.cuda.synchronize()
    return frames


def check_batch(oracle, frames, data, m, epi, tp=None, bad=()):
    """every frame against the oracle; frames listed in `bad` must carry ERR_RANGE and no output"""
    otp = oracle_tri_params(oracle, KITTI)
    if tp is not None:
        otp.minimum_disparity_pixels = tp.minimum_disparity_pixels
    n_matched = 0
    for b, fr in enumerate(data):
        status = int(frames.status[b].item())
        if b in bad:
            assert status == ops._lib.ERR_RANGE and int(frames.n_matches[b].item()) == 0, "frame %d" % b
            if epi:
                assert int(frames.n_fixed[b].item()) == 0, "frame %d" % b
            continue
        ref, rflags = oracle.stereo_match(fr["uv_left"], fr["desc_left"], fr["uv_right"], fr["desc_right"], oracle_stereo_params(oracle, m))
        got = frames.matches_of(b)
        assert corr_equal(ref, got), "frame %d: %d vs %d correspondences" % (b, len(ref), len(got))
        assert status == rflags, "frame %d" % b
        n_matched += len(ref)
        if epi:
            uvuv, src = oracle.stereo_assemble(fr["uv_left"], fr["uv_right"], ref)
            nf = int(frames.n_fixed[b].item())
            assert nf == len(uvuv), "frame %d" % b
            assert np.array_equal(frames.fixed_uvuv[b, :nf].cpu().numpy().view(np.uint32), uvuv.view(np.uint32)), "frame %d" % b
            assert np.array_equal(frames.fixed_desc[b, :nf].cpu().numpy(), fr["desc_left"][src]), "frame %d" % b
            xyz, valid = oracle.triangulate(uvuv, otp)
            g = frames.fixed_xyz[b, :nf].cpu().numpy()
            assert np.array_equal(g[:, :3].view(np.uint32), xyz.view(np.uint32)), "frame %d" % b
            assert np.array_equal(g[:, 3] != 0, valid.astype(bool)), "frame %d" % b
    return n_matched


def kitti_like(seed, n, rows=376, jitter=0.15):
    """a KITTI-shaped pair of n keypoints per image, its rows stretched onto `rows` image rows"""
    if n == 0:
        return {"uv_left": np.zeros((0, 2), np.float32), "desc_left": np.zeros((0, 32), np.uint8),
                "uv_right": np.zeros((0, 2), np.float32), "desc_right": np.zeros((0, 32), np.uint8)}
    rng = np.random.default_rng(seed)
    fr = syn.stereo_frame(rng, KITTI, n, row_jitter_fraction=jitter, visible_fraction=0.5)
    fr = {k: fr[k] for k in ("uv_left", "desc_left", "uv_right", "desc_right")}
    if rows != 376:
        for k in ("uv_left", "uv_right"):
            fr[k] = fr[k].copy()
            fr[k][:, 1] = np.minimum(np.floor(fr[k][:, 1] * (rows / 376.0)), rows - 1) + 0.5
    return fr


def _pool_cap(stride, rows):
    return sd.v5_layout(stride, rows)["pool_cap"]


def _demand(fr, m, rows):
    _, _, passes = sr.match(fr["uv_left"], fr["desc_left"], fr["uv_right"], fr["desc_right"], m["maximum_descriptor_distance"],
                            m["maximum_distance_ratio_to_second_best"], m["minimum_matching_ratio"], m["maximum_disparity_pixels"],
                            m["epipolar_line_thickness_pixels"], passes=True) if len(fr["uv_left"]) <= 1200 else (None, None, None)
    return sd.window_demand(fr["uv_left"], fr["uv_right"], m["maximum_disparity_pixels"], m["epipolar_line_thickness_pixels"], rows, passes)


# ---- parity table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", DISPATCH, ids=[r["id"] for r in DISPATCH])
def test_dispatch_row_matches_oracle(oracle, make_ctx, row):
    m = dict(M_KITTI, epipolar_line_thickness_pixels=row["thickness"])
    _assert_variant(_expect(row["stride"], 376, m, row["epi"], row.get("v3", 0), row.get("unstaged", 0)), row["kernel"], row["args"])
    ctx = make_ctx(row.get("v3", 0), row.get("unstaged", 0))
    data = [kitti_like(1000 * len(row["id"]) + 17 * b + row["stride"], n, jitter=0.2 if row["thickness"] else 0.0) for b, n in enumerate(row["n"])]
    frames = run_batch(ctx, m, 376, data, row["stride"], row["epi"], expect=(row["kernel"], row["args"]))
    assert check_batch(oracle, frames, data, m, row["epi"]) > 300


# ---- shape limits and layout fallbacks -------------------------------------------------------------------------------------------
SHAPES = [  # stride, image rows, thickness -> instantiation
    (1024, 376, 0, "stereo_match5_kernel", "1,false,true"),
    (1025, 376, 0, "stereo_match5_kernel", "2,false,true"),
    (2048, 376, 1, "stereo_match5_kernel", "2,true,true"),
    (2049, 376, 0, "stereo_match_kernel", "4,false"),
    (4096, 376, 1, "stereo_match_kernel", "4,false"),
    (4097, 376, 0, "stereo_match_kernel", "8,false"),
    (8192, 376, 1, "stereo_match_kernel", "8,false"),
    (64, 4096, 1, "stereo_match5_kernel", "1,true,true"),     # the tallest image: v5, looped scans, four rows per chain lane
    (256, 376, 120, "stereo_match5_kernel", "1,true,true"),   # the thickest epipolar line: 241 passes
    (2048, 492, 0, "stereo_match5_kernel", "2,false,true"),   # the last row count whose v5 layout fits (pool_cap 0)
    (2048, 493, 0, "stereo_match_kernel", "2,true"),          # v5 LDS over 160 KiB
    (2047, 2047, 0, "stereo_match_kernel", "2,true"),         # cap 8188 passes its check, the layout does not fit
    (2048, 2048, 1, "stereo_match_kernel", "2,true"),         # cap 8192: refused by the 13-bit check
]


@pytest.mark.parametrize("stride,rows,thickness,kernel,args", SHAPES, ids=["%dx%d_t%d" % s[:3] for s in SHAPES])
def test_shape_edges(oracle, make_ctx, stride, rows, thickness, kernel, args):
    m = dict(M_KITTI, epipolar_line_thickness_pixels=thickness)
    d = _expect(stride, rows, m, 1)
    _assert_variant(d, kernel, args)
    if (stride, rows) == (2048, 492):
        assert d["v5"]["pool_cap"] == 0
    if (stride, rows) == (2048, 493):
        assert d["v5_why"] == "lds"
    if (stride, rows) == (2047, 2047):
        assert d["v5"]["cap"] == sd.V5_CAP_MAX and d["v5_why"] == "lds"
    if (stride, rows) == (2048, 2048):
        assert d["v5"]["cap"] == sd.V5_CAP_MAX + 4 and d["v5_why"] == "cap"
    ctx = make_ctx()
    ns = [stride, max(1, stride // 2 + 1), min(stride, 37)]
    data = [kitti_like(stride + rows + b, n, rows, jitter=0.2 if thickness else 0.0) for b, n in enumerate(ns)]
    frames = run_batch(ctx, m, rows, data, stride, 1, expect=(kernel, args))
    assert check_batch(oracle, frames, data, m, 1) > min(stride, 300) // 3


@pytest.mark.parametrize("stride,rows,thickness", [(8193, 376, 0), (1024, 4097, 0), (1024, 376, 121), (0, 376, 0), (1024, 0, 0)])
def test_shape_refusals(make_ctx, stride, rows, thickness):
    m = dict(M_KITTI, epipolar_line_thickness_pixels=thickness)
    assert _expect(stride, rows, m, 1)["refused"] in ("shape", "thickness")
    ctx = make_ctx()
    frames = ops.StereoFrames(0, 1, max(stride, 1), epilogue=True)
    with pytest.raises(ops.ProslamHipError) as ei:
        frames.stride = stride
        ops.stereo_match_batch(ctx, ops.stereo_params(m, rows), frames, _tri())
    assert ei.value.status == ops._lib.ERR_UNSUPPORTED


# ---- the acceptance table: thresholds, ratio > 1, second best 0 ------------------------------------------------------------------
def _threshold_frame(seed, rows=376):
    rng = np.random.default_rng(seed)
    fb = sr.FrameBuilder(rng)
    row = 0
    for d in (250, 253, 254, 255, 256, 255, 256, 254):  # lone candidates: the distance threshold alone decides
        for col in (100, 400, 700, 1000):
            fb.window(row, col + d % 7, [d])
        row += 1
    for dists in ([255, 256], [256, 255], [254, 255, 256], [256, 256], [255, 255, 255, 255, 256], [256, 254, 255, 256, 256, 255]):
        for col in (100, 400, 700, 1000):
            fb.window(row, col, dists)
        row += 1
    return fb.build()


@pytest.mark.parametrize("max_dist,kernel,args", [(255.0, "stereo_match5_kernel", "1,false,true"), (255.5, "stereo_match_kernel", "1,true"),
                                                  (256.0, "stereo_match_kernel", "1,true"), (256.5, "stereo_match_kernel", "1,true")])
def test_distance_threshold_edges(oracle, make_ctx, max_dist, kernel, args):
    m = dict(M_EDGE, maximum_descriptor_distance=max_dist, maximum_distance_ratio_to_second_best=1.5)
    _assert_variant(_expect(1024, 376, m, 1), kernel, args)
    assert sd.fill_accept_table(max_dist, 1.5)[0] == {255.0: 255, 255.5: 256, 256.0: 256, 256.5: 257}[max_dist]
    ctx = make_ctx()
    data = [_threshold_frame(s) for s in (1, 2, 3)]
    frames = run_batch(ctx, m, 376, data, 1024, 1)
    assert check_batch(oracle, frames, data, m, 1) > 20
    # the last distance accepted is the threshold's edge
    resp = np.concatenate([frames.matches_of(b)["response"] for b in range(3)])
    assert resp.max() == {255.0: 254.0, 255.5: 255.0, 256.0: 255.0, 256.5: 256.0}[max_dist]


def _ratio_frame(seed):
    rng = np.random.default_rng(seed)
    fb = sr.FrameBuilder(rng)
    row = 0
    for dists in ([0, 0], [0, 0, 0, 0, 0, 0], [5, 5], [4, 4, 4, 4, 4, 4], [0, 7], [9, 9, 9], [3, 2], [6, 6, 6, 6, 6, 6, 6, 6, 2], [1, 0, 0],
                  [0, 3, 0, 3, 3, 3]):
        for col in (50, 300, 600, 900):
            fb.window(row, col, dists)
        row += 1
    return fb.build()


@pytest.mark.parametrize("v3", [0, 1])
def test_ratio_above_one_and_second_best_zero(oracle, make_ctx, v3):
    m = dict(M_EDGE, maximum_distance_ratio_to_second_best=1.5)
    _, bmax = sd.fill_accept_table(m["maximum_descriptor_distance"], 1.5)
    assert bmax[0] == -1 and bmax[5] == 7
    _assert_variant(_expect(1024, 376, m, 1, v3), *(("stereo_match_kernel", "1,true") if v3 else ("stereo_match5_kernel", "1,false,true")))
    ctx = make_ctx(v3)
    data = [_ratio_frame(s) for s in (4, 5)]
    dem = sd.window_demand(data[0]["uv_left"], data[0]["uv_right"], m["maximum_disparity_pixels"], 0, 376)
    assert dem[0]["largest"] > 4 and dem[0]["total"] <= _pool_cap(1024, 376)
    frames = run_batch(ctx, m, 376, data, 1024, 1)
    assert check_batch(oracle, frames, data, m, 1) > 10


# ---- the candidate pool -------------------------------------------------------------------------------------------------------
def _edge_window_frame(seed, size, rows=376, col0=0):
    """windows of `size` candidates whose best distance equals bmax[second] (ratio 0.8: best 7, second 10) at every position, and
    windows one distance short of or over it; -> (frame, builder indices of the left keypoints that sit exactly on the edge)"""
    rng = np.random.default_rng(seed)
    fb = sr.FrameBuilder(rng)
    edge, n_windows = [], 1000 // size  # right keypoints within the stride
    for w in range(n_windows):
        k, j = divmod(w, 19)
        row, col = (k * 7) % rows, col0 + 40 + 60 * j
        tail = [int(x) for x in rng.integers(20, 90, size - 2)]
        pos = (k + j) % size
        kind = (k + 2 * j) % 3
        best = (7, 6, 8)[kind]
        dists = tail[:]
        dists.insert(pos, best)
        dists.insert((pos + 1 + j) % size, 10)
        i = fb.window(row, col, dists[:size], keep=(j % 4 != 3))
        if kind == 0:
            edge.append(i)
    fr = fb.build()
    return fr, [int(fb.left_index[i]) for i in edge]


@pytest.mark.parametrize("size", [4, 5, 9])
@pytest.mark.parametrize("v3", [0, 1])
def test_acceptance_edge_in_windows_of_four_and_more(oracle, make_ctx, size, v3):
    """best == bmax[second] is accepted: in the four-candidate verdict table (size 4), in the pooled sweep (size 5, 9)"""
    m = dict(M_EDGE)
    _, bmax = sd.fill_accept_table(m["maximum_descriptor_distance"], m["maximum_distance_ratio_to_second_best"])
    assert bmax[10] == 7
    ctx = make_ctx(v3)
    data, edges = [], []
    for s in (size, size + 10):
        fr, e = _edge_window_frame(s, size)
        data.append(fr)
        edges.append(e)
    dem = sd.window_demand(data[0]["uv_left"], data[0]["uv_right"], m["maximum_disparity_pixels"], 0, 376)[0]
    if size == 4:
        assert dem["windows"] == []
    else:
        assert dem["largest"] == size and 0 < dem["total"] <= _pool_cap(1024, 376)
    frames = run_batch(ctx, m, 376, data, 1024, 1)
    check_batch(oracle, frames, data, m, 1)
    for b in range(2):
        got = frames.matches_of(b)
        on_edge = dict(zip(got["fixed_idx"].tolist(), got["response"].tolist()))
        assert all(on_edge.get(i) == 7.0 for i in edges[b]), "frame %d: a best distance equal to bmax[second] was not accepted" % b


POOL_CASES = [  # id, stride, rows, thickness, frame shape (rows used, left / right per row, span), expected pool state
    ("partly_t0", 1024, 376, 0, (40, 8, 10, 14), "partly"),
    ("partly_t2", 1024, 376, 2, (40, 8, 10, 14), "partly"),
    ("exhausted_t0", 2048, 480, 0, (60, 12, 16, 18), "exhausted"),
    ("exhausted_t1", 2048, 480, 1, (60, 12, 16, 18), "exhausted"),
    ("exhausted_t3", 2000, 376, 3, (70, 14, 16, 12), "exhausted"),
    ("cap64_t0", 2048, 489, 0, (40, 10, 12, 14), "exhausted"),
    ("cap64_t1", 2048, 489, 1, (40, 10, 12, 14), "exhausted"),
    ("cap0_t0", 2048, 490, 0, (40, 10, 12, 14), "none"),
    ("cap0_t2", 2048, 490, 2, (40, 10, 12, 14), "none"),
    ("cap72_tall", 1000, 2094, 1, (50, 8, 10, 12), "exhausted"),
    ("cap0_tall", 1000, 2095, 0, (50, 8, 10, 12), "none"),
]


@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_candidate_pool(oracle, make_ctx, case):
    cid, stride, rows, thickness, shape, state = case
    m = dict(M_EDGE, maximum_disparity_pixels=14, epipolar_line_thickness_pixels=thickness)
    d = _expect(stride, rows, m, 1)
    assert d["kernel"] == "stereo_match5_kernel", d
    cap = d["v5"]["pool_cap"]
    assert cap == {"cap64": 64, "cap0_": 0, "cap72": 72}.get(cid[:5], cap)
    ctx = make_ctx()
    data = []
    for b in range(3):
        rng = np.random.default_rng(sum(map(ord, cid)) + b)
        n_rows = shape[0] - 10 * b
        first = int(rng.integers(0, rows - n_rows))  # adjacent rows: the later passes of a thick line find crowded windows too
        fr = sr.crowded_frame(rng, rows, n_rows, shape[1], shape[2], shape[3], jitter=0.3 if thickness else 0.0,
                              row_list=np.arange(first, first + n_rows), col0=300 + 40 * b)
        assert len(fr["uv_left"]) <= stride and len(fr["uv_right"]) <= stride
        dem = _demand(fr, m, rows)
        if state == "partly":
            assert all(0 <= p["total"] <= cap for p in dem) and dem[0]["total"] > 0
            if thickness:
                assert dem[1]["total"] + dem[2]["total"] > 0  # later passes use the pool too
        elif state == "exhausted":
            assert 0 < cap < dem[0]["total"]  # the replay sweep runs in the first pass
        else:
            assert cap == 0 and dem[0]["largest"] > 4  # every crowded window is replayed
        data.append(fr)
    frames = run_batch(ctx, m, rows, data, stride, 1)
    assert check_batch(oracle, frames, data, m, 1) > 50


# ---- scans, padding, tall images ----------------------------------------------------------------------------------------------
def _row_pattern_frame(seed, rows, stride):
    """row r holds r % 4 + 4 * (r % 3 == 0) keypoints (lengths = 0, 1, 2, 3 mod 4), every fifth row none, a full row of 20 after
    every empty one"""
    rng = np.random.default_rng(seed)
    counts = np.array([0 if r % 5 == 4 else (20 if r % 5 == 0 and r else r % 4 + 4 * (r % 3 == 0)) for r in range(rows)])
    while counts.sum() > stride:
        counts[rng.integers(0, rows)] = 0
    bank = rng.integers(0, 256, (9, 32), dtype=np.uint8)
    uvl, uvr = [], []
    for r, c in enumerate(counts):
        if c:
            cols = rng.integers(0, 1200, c) + 0.5
            uvl += [(u + rng.integers(0, 12), r + 0.5) for u in cols]
            uvr += [(u, r + 0.3) for u in cols]
    n = len(uvl)
    base = bank[rng.integers(0, 9, n)]
    dl = np.bitwise_xor(base, np.packbits(rng.random((n, 256)) < 0.03, axis=1))
    dr = np.bitwise_xor(base, np.packbits(rng.random((n, 256)) < 0.03, axis=1))
    pl, pr = rng.permutation(n), rng.permutation(n)
    return {"uv_left": np.asarray(uvl, np.float32)[pl], "desc_left": dl[pl], "uv_right": np.asarray(uvr, np.float32)[pr], "desc_right": dr[pr]}, counts


@pytest.mark.parametrize("rows,stride,thickness", [(511, 1024, 0), (512, 1024, 1), (513, 1024, 0), (514, 1024, 1), (1100, 1024, 1),
                                                   (2094, 1000, 0), (4096, 512, 1)])
@pytest.mark.parametrize("v3", [0, 1])
def test_scan_branches_and_sentinel_padding(oracle, make_ctx, rows, stride, thickness, v3):
    """chunk = ceil(rows / 64) <= 8 unrolls the v5 scans, > 8 loops (rows >= 513; the first generation's row-start scan covers
    rows + 1 entries and loops from rows 512); rows > 1024 give every chain lane several rows"""
    m = dict(M_EDGE, maximum_disparity_pixels=12, epipolar_line_thickness_pixels=thickness)
    d = _expect(stride, rows, m, 1, v3)
    assert d["kernel"] == ("stereo_match_kernel" if v3 else "stereo_match5_kernel"), d
    chunk = (rows + 63) // 64
    assert (chunk > 8) == (rows >= 513)
    ctx = make_ctx(v3)
    data, counts = [], []
    for b in range(2):
        fr, c = _row_pattern_frame(rows + 31 * b, rows, stride)
        data.append(fr)
        counts.append(c)
    assert {int(x) % 4 for x in counts[0] if x} == {0, 1, 2, 3} and (counts[0] == 0).any()
    frames = run_batch(ctx, m, rows, data, stride, 1)
    assert check_batch(oracle, frames, data, m, 1) > 100


# ---- the coordinate domain ------------------------------------------------------------------------------------------------------
def _coords_frame(seed, rows, u=None, v=None, side="left"):
    """a 200-keypoint frame with a few right-column keypoints; keypoint 5 of `side` gets (u, v) when given"""
    fr = kitti_like(seed, 200, rows, jitter=0.0)
    rng = np.random.default_rng(seed)
    for k in ("uv_left", "uv_right"):
        fr[k] = fr[k].copy()
        fr[k][:12, 0] = np.float32(32767.0) + rng.random(12).astype(np.float32) * 0.99  # column 32767: the window's top bound
        fr[k][:12, 1] = np.float32(3.5)
    fr["desc_right"] = fr["desc_right"].copy()
    fr["desc_right"][:12] = syn.flip_bits(rng, fr["desc_left"][:12], 0.02)
    if u is not None:
        fr["uv_" + side][5, 0] = u
    if v is not None:
        fr["uv_" + side][5, 1] = v
    return fr


@pytest.mark.parametrize("v3", [0, 1])
def test_coordinate_domain(oracle, make_ctx, v3):
    rows = 376
    f32 = np.float32
    below_max_u = np.nextafter(f32(32768.0), f32(0.0))
    below_rows = np.nextafter(f32(rows), f32(0.0))
    tiny_negative = np.nextafter(f32(0.0), f32(-1.0))
    accepted = [dict(u=f32(32767.0)), dict(u=f32(32767.5)), dict(u=below_max_u), dict(u=below_max_u, side="right"),
                dict(v=below_rows), dict(v=below_rows, side="right"), dict(u=f32(-0.0)), dict(v=f32(-0.0), side="right"), dict()]
    refused = [dict(u=f32(32768.0)), dict(u=f32(32768.0), side="right"), dict(v=f32(rows)), dict(v=f32(rows), side="right"),
               dict(u=tiny_negative), dict(v=tiny_negative, side="right"), dict(u=f32(np.nan)), dict(v=f32(np.nan), side="right"),
               dict(u=f32(np.inf))]
    data, bad = [], set()
    for k in range(max(len(accepted), len(refused))):  # refused frames between accepted ones
        if k < len(accepted):
            data.append(_coords_frame(300 + k, rows, **accepted[k]))
        if k < len(refused):
            bad.add(len(data))
            data.append(_coords_frame(400 + k, rows, **refused[k]))
    m = dict(M_KITTI, epipolar_line_thickness_pixels=1)
    assert _expect(256, rows, m, 1, v3)["kernel"] == ("stereo_match_kernel" if v3 else "stereo_match5_kernel")
    ctx = make_ctx(v3)
    frames = run_batch(ctx, m, rows, data, 256, 1)
    check_batch(oracle, frames, data, m, 1, bad=bad)
    # the keypoints on column 32767 are matched
    assert sum(int((frames.matches_of(b)["fixed_idx"] < 12).sum()) for b in range(len(data)) if b not in bad) > 20


# ---- the persistent grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v3,thickness", [(0, 0), (0, 1), (1, 1)])
def test_persistent_grid_frames_strided_over_cus(oracle, make_ctx, v3, thickness):
    """more frames than CUs: the workgroup of frame k also takes k + CUs (and k + 2 CUs); pool-exhausting frames before
    pool-using ones, an ERR_RANGE frame before a crowded valid one, empty frames on either side, counts varying under one stride"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    stride, rows = 2048, 480
    m = dict(M_EDGE, maximum_disparity_pixels=14, epipolar_line_thickness_pixels=thickness)
    d = _expect(stride, rows, m, 1, v3)
    assert d["kernel"] == ("stereo_match_kernel" if v3 else "stereo_match5_kernel") and (v3 or d["args"].startswith("2,"))
    assert v3 or d["v5"]["pool_cap"] == 248
    n_frames = 2 * cus + 7
    empty = {"uv_left": np.zeros((0, 2), np.float32), "desc_left": np.zeros((0, 32), np.uint8)}
    kinds, data, bad = [], [], set()
    for f in range(n_frames):
        # frame f and frame f + CUs run on one workgroup, one after the other
        k = f % 6 if f < cus else (f - cus) % 6
        rng = np.random.default_rng(5000 + f)
        if f < cus:
            kind = ("exhausting", "range", "exhausting", "empty_left", "using", "empty_right")[k]
        else:
            kind = ("using", "crowded", "exhausting", "using", "empty_left", "crowded")[k]
        if kind == "exhausting":
            fr = sr.crowded_frame(rng, rows, 50 + k, 12, 16, 18, jitter=0.3 if thickness else 0.0)
        elif kind == "using":
            fr = sr.crowded_frame(rng, rows, 2 + f % 3, 6, 8, 12, jitter=0.3 if thickness else 0.0)
        elif kind == "crowded":
            fr = sr.crowded_frame(rng, rows, 6 + f % 5, 6, 8, 12, jitter=0.3 if thickness else 0.0)
        else:
            fr = sr.crowded_frame(rng, rows, 8 + f % 3, 5, 6, 12)
        if kind == "range":
            fr["uv_left"] = fr["uv_left"].copy()
            fr["uv_left"][f % len(fr["uv_left"]), 1] = rows
            bad.add(f)
        if kind == "empty_left":
            fr = dict(fr, **empty)
        if kind == "empty_right":
            fr = dict(fr, uv_right=empty["uv_left"], desc_right=empty["desc_left"])
        kinds.append(kind)
        data.append(fr)
    if not v3:
        cap = d["v5"]["pool_cap"]
        for f in range(n_frames):
            if kinds[f] == "exhausting":
                assert sd.window_demand(data[f]["uv_left"], data[f]["uv_right"], 14, thickness, rows)[0]["total"] > cap
        for f in range(cus, n_frames):
            if kinds[f] == "using":
                tot = sd.window_demand(data[f]["uv_left"], data[f]["uv_right"], 14, 0, rows)[0]["total"]
                assert 0 < tot <= cap, (f, tot)
    assert kinds[0] == "exhausting" and kinds[cus] == "using" and kinds[1] == "range" and kinds[1 + cus] == "crowded"
    assert kinds[3] == "empty_left" and kinds[5] == "empty_right"
    assert len({len(fr["uv_left"]) for fr in data}) > 8
    ctx = make_ctx(v3)
    frames = run_batch(ctx, m, rows, data, stride, 1)
    check_batch(oracle, frames, data, m, 1, bad=bad)


# ---- triangulation against float64 ---------------------------------------------------------------------------------------------
def triangulate_f64(uvuv, tp):
    """triangulator_rigid_stereo.cpp:39-45 (the disparity gate) and triangulateRectifiedMidpoint (:60-85) in float64 on the float32
    inputs and parameters the kernel reads -> (xyz [n, 3], valid [n], error bound [n, 3])"""
    f = lambda x: float(np.float32(x))  # noqa: E731
    fx, fy, cx, cy, bx, md, inf = (f(tp.fx), f(tp.fy), f(tp.cx), f(tp.cy), f(tp.b_x), f(tp.minimum_disparity_pixels), f(tp.infinity_depth_meters))
    q = np.asarray(uvuv, dtype=np.float64)
    xl, yl, xr, yr = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    disp = xl - xr
    valid = ~(disp < md)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(xl > xr, bx / np.where(xl > xr, disp, 1.0), inf)
    x = 1.0 / fx * (xl - cx) * depth
    y = 1.0 / fy * ((yl + yr) / 2 - cy) * depth
    # float32 evaluation, first order in u: the disparity rounds once and the division once (depth: 2u); x adds 1 / fx, the
    # subtraction and two products (4 roundings on top of depth's 2); y the sum, the subtraction, 1 / fy and two products (5).  The
    # subtractions are bounded by the magnitudes of their operands (cancellation), and one more u per bound covers second order terms.
    ez = 3 * U * np.abs(depth)
    ex = 7 * U * abs(1.0 / fx) * (np.abs(xl) + abs(cx)) * np.abs(depth)
    ey = 8 * U * abs(1.0 / fy) * ((np.abs(yl) + np.abs(yr)) / 2 + abs(cy)) * np.abs(depth)
    xyz = np.where(valid[:, None], np.stack([x, y, depth], axis=1), 0.0)
    return xyz, valid, np.where(valid[:, None], np.stack([ex, ey, ez], axis=1), 0.0)


def _disparity_frame(seed, min_disp):
    """matches whose disparities sit at minimum_disparity_pixels, one coordinate step above and below it, at zero, and spread
    over the image; columns within a factor of two of each other keep the float32 disparity exact"""
    rng = np.random.default_rng(seed)
    fb = sr.FrameBuilder(rng)
    step = 2.0 ** -16  # coordinate step of floats in [128, 256)
    disps = [min_disp, min_disp + step, min_disp - step, 0.0, 0.0, min_disp + 2 * step, 3.0, 17.25, 0.5, 1.0 - step, 1.0, 1.0 + step]
    row = 0
    for k in range(30):
        for j, dd in enumerate(disps):
            xl = np.float32(140.0 + 9 * j + rng.random())
            xr = np.float32(xl - np.float32(dd))
            assert float(xl) - float(xr) == float(np.float32(dd)) or dd > 16
            base = rng.integers(0, 256, 32, dtype=np.uint8)
            fb.left(float(xl), row + 0.5, base)
            fb.right(float(xr), row + (0.5 if j % 2 else 0.25), sr.at_distance(rng, base, 3))
        row += 1
    fr = fb.build()
    cfg_rng = np.random.default_rng(seed + 1)
    kitti = syn.stereo_frame(cfg_rng, KITTI, 600, visible_fraction=0.9)
    for k in ("uv_left", "desc_left", "uv_right", "desc_right"):
        extra = kitti[k]
        if k.startswith("uv"):
            extra = extra.copy()
            extra[:, 1] = np.minimum(extra[:, 1], 375.0)
            extra[:, 1] = np.where(extra[:, 1] < 40, extra[:, 1] + 40, extra[:, 1])  # below the crafted rows
        fr[k] = np.concatenate([fr[k], extra])
    return fr


def _check_f64(uvuv, got_xyz4, tp):
    xyz, valid, bound = triangulate_f64(uvuv, tp)
    assert np.array_equal(got_xyz4[:, 3] != 0, valid), "validity differs from the float64 gate"
    g = got_xyz4[:, :3].astype(np.float64)
    assert np.all(np.isfinite(g))
    err = np.abs(g - xyz)
    assert np.all(err <= bound), "worst excess %.3g" % np.max(err - bound)
    return valid


@pytest.mark.parametrize("min_disp", [1.0, 0.0])
@pytest.mark.parametrize("v3", [0, 1])
def test_epilogue_points_vs_float64(oracle, make_ctx, min_disp, v3):
    m = dict(M_KITTI, maximum_disparity_pixels=120)
    tp = _tri(min_disp)
    ctx = make_ctx(v3)
    data = [_disparity_frame(s, min_disp) for s in (31, 32)]
    assert max(len(fr["uv_left"]) for fr in data) <= 1024
    frames = run_batch(ctx, m, 376, data, 1024, 1, tp)
    check_batch(oracle, frames, data, m, 1, tp=tp)
    seen = set()
    for b in range(len(data)):
        nf = int(frames.n_fixed[b].item())
        uvuv = frames.fixed_uvuv[b, :nf].cpu().numpy()
        valid = _check_f64(uvuv, frames.fixed_xyz[b, :nf].cpu().numpy(), tp)
        disp = uvuv[:, 0].astype(np.float64) - uvuv[:, 2]
        seen |= {("at", bool(v)) for d, v in zip(disp, valid) if d == min_disp}
        seen |= {("zero", bool(v)) for d, v in zip(disp, valid) if d == 0.0}
        seen |= {("below", bool(v)) for d, v in zip(disp, valid) if min_disp - 2.0 ** -15 < d < min_disp}
        seen |= {("above", bool(v)) for d, v in zip(disp, valid) if min_disp < d < min_disp + 2.0 ** -15}
        if min_disp == 0.0:
            z = frames.fixed_xyz[b, :nf, 2].cpu().numpy()
            assert np.all(z[disp == 0.0] == np.float32(tp.infinity_depth_meters))  # the infinity depth
    assert ("at", True) in seen and ("above", True) in seen and (min_disp <= 0.0 or ("below", False) in seen)
    assert ("zero", min_disp <= 0.0) in seen


def test_standalone_triangulator_vs_float64(hip_ctx):
    rng = np.random.default_rng(77)
    pts = syn.sample_landmarks(rng, KITTI["camera"], KITTI["depth"], 4000)
    u, v, ur = syn.project_left_right(KITTI["camera"], pts)
    uvuv = np.stack([u, v, ur, v + rng.integers(-1, 2, 4000)], axis=1).astype(np.float32)
    # left columns >= 2: a disparity near the gate is then a difference of floats within a factor of two (exact in float32)
    uvuv = uvuv[uvuv[:, 0] >= 2.0]
    uvuv[::9, 2] = uvuv[::9, 0]                                   # zero disparity
    uvuv[1::9, 2] = uvuv[1::9, 0] - np.float32(1.0)               # at the gate (exact where the columns allow)
    uvuv[2::9, 2] = np.nextafter(uvuv[2::9, 0] - np.float32(1.0), np.float32(-np.inf))
    for min_disp in (1.0, 0.0):
        tp = _tri(min_disp)
        xyz, valid = ops.triangulate(hip_ctx, tp, uvuv)
        _check_f64(uvuv, np.concatenate([xyz, valid[:, None].astype(np.float32)], axis=1), tp)
