"""The per-frame caches of the split pipeline's search kernel (csrc/align.hip): the first search of a frame loop leaves an image
of the lattice and the fixed descriptor rows in lattice order in global memory, the later searches stream both back instead of
gathering the rows through the lattice again.

Every case runs the split pipeline and compares it bit for bit with the CPU checker and with the fused kernel (PRS_FUSED_ALIGN=1),
which keeps everything in LDS and uses no cache: correspondences in order incl. response bits, pose bits, finder state (radius,
distance, iteration, number of searches, convergence latch, both transforms), status / warnings / counts, mean disparity.  The
cases are the ones a stale or misplaced cache entry would break: tiny and full fixed clouds in one batch, frames that need a fifth
search next to frames that are done after four, a context reused for other clouds and for another max_fixed, a captured graph
replayed on inputs overwritten in place, every search pattern, the eight-slot instantiation and the unpruned scan.  The first
search also binds the mean disparity while it builds the lattice -- as an exact integer sum where the disparities allow it, as the
reference's chain of float additions otherwise: both sides of every condition of that choice."""
import numpy as np
import pytest

from helpers import make_align_case
from srrg2_proslam_amd import configs, ops
from test_align_dispatch_gpu import _bits, _check_frame, _context, _correlated_frame, _device_params, _oracle_frame, _run_batch

pytestmark = pytest.mark.gpu


def _case(oracle, cfg_name, seed, n_kp, keep=None, sigma_t=0.05, sigma_r=0.003, n_moving=None):
    cfg, fixed, dfix, mp, T, X0 = make_align_case(cfg_name, seed, n_kp, n_moving or n_kp, sigma_t=sigma_t, sigma_r=sigma_r)
    keep = len(fixed) if keep is None else keep
    assert len(fixed) >= keep
    return dict(fixed=fixed[:keep].copy(), dfix=dfix[:keep].copy(), xyz=mp["xyz"], dmov=mp["desc"], scale=oracle.info_scale_from_nopt(mp["n_opt"]), X0=X0)


def _snapshot(frames):
    """everything a frame loop leaves behind, as comparable values"""
    out = []
    for b in range(frames.batch):
        n = int(frames.n_corr[b].item())
        st, res = frames.state_of(b), frames.result_of(b)
        out.append(dict(
            corr=frames.corr[b, :n].cpu().numpy().copy(),  # (fixed index, moving index, response bits) in order
            X=_bits(frames.X[b].cpu().numpy()).copy(),
            state=(int(st.search_radius_pixels), int(st.current_iteration), _bits([st.descriptor_distance]).tolist(), st.has_converged, st.config_changed,
                   st.num_recomputes, _bits(list(st.local_map_in_sensor)).tolist(), _bits(list(st.local_map_in_sensor_previous)).tolist()),
            # (not the prune hint in `reserved`: it counts queries that overflowed their survivor slots, the fused kernel has four
            # slots where the search half may have eight, and no result depends on it)
            result=(res.status, res.warnings, res.num_inliers, res.num_outliers, res.num_invalid, res.num_correspondences, res.iterations,
                    _bits([res.mean_disparity]).tolist())))
    return out


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["corr"], w["corr"]), "%s frame %d: correspondences (%d vs %d)" % (what, b, len(g["corr"]), len(w["corr"]))
        assert np.array_equal(g["X"], w["X"]), "%s frame %d: pose bits" % (what, b)
        assert g["state"] == w["state"], "%s frame %d: finder state %s vs %s" % (what, b, g["state"][:6], w["state"][:6])
        assert g["result"] == w["result"], "%s frame %d: result %s vs %s" % (what, b, g["result"], w["result"])


def _against_oracle(oracle, cfg, frames, cases, fkw, what):
    searches = []
    for b, c in enumerate(cases):
        of, res, rcorr = _oracle_frame(oracle, cfg, c, fkw, {})
        _check_frame(frames, b, of, res, rcorr, "%s frame %d" % (what, b))
        assert frames.state_of(b).num_recomputes == of.num_recomputes, "%s frame %d: number of searches" % (what, b)
        searches.append(of.num_recomputes)
    return searches


def _split_and_fused(oracle, monkeypatch, cfg, cases, max_fixed, fkw, what, no_prefilter=0):
    """the batch through the split pipeline (against the checker) and through the fused kernel (against the split pipeline)"""
    ctx = _context(monkeypatch, no_prefilter=no_prefilter)
    try:
        frames = _run_batch(ctx, cfg, cases, max_fixed, fkw, {})
        searches = _against_oracle(oracle, cfg, frames, cases, fkw, what)
        split = _snapshot(frames)
    finally:
        ctx.close()
    ctx = _context(monkeypatch, fused=1, no_prefilter=no_prefilter)
    try:
        fused = _snapshot(_run_batch(ctx, cfg, cases, max_fixed, fkw, {}))
    finally:
        ctx.close()
    _assert_same(split, fused, what + " split vs fused")
    return split, searches


SMALL = (0, 1, 15, 16, 17)


@pytest.mark.parametrize("search_type", [0, 1, 2, 3], ids=["kdtree", "square", "circle", "rhombus"])
def test_tiny_and_full_fixed_clouds_in_one_batch(oracle, monkeypatch, search_type):
    """0, 1, 15, 16, 17 fixed points (no, one partial, one full and one full + one partial 16-byte group of the streamed arrays)
    next to frames with exactly max_fixed points, one of them with its last lattice entry in the last cell a search scans; square,
    circle and rhombus stream the cached rows back, the KD-tree finder keeps its own path"""
    cfg = configs.get("kitti")
    max_fixed = 700
    rng = np.random.default_rng(8100 + search_type)
    cases = [_case(oracle, "kitti", 8200 + k, 600, keep=k) for k in SMALL]
    cases.append(_case(oracle, "kitti", 8300, 1300, keep=max_fixed))
    corner = _correlated_frame(rng, cfg, max_fixed, corner=True)
    assert tuple(corner["fixed"][-1, :2]) == (cfg["camera"]["cols"] - 1, cfg["camera"]["rows"] - 1)
    cases.append(corner)
    fkw = dict(search_type=search_type, maximum_search_radius_pixels=100)
    split, searches = _split_and_fused(oracle, monkeypatch, cfg, cases, max_fixed, fkw, "pattern %d" % search_type)
    assert [len(c["fixed"]) for c in cases] == list(SMALL) + [max_fixed, max_fixed]
    assert min(searches) >= 2  # every frame went through later searches, i.e. through the cache
    assert len(split[5]["corr"]) > 100 and len(split[6]["corr"]) > 50


def test_frames_done_after_four_searches_next_to_frames_that_need_a_fifth(oracle, monkeypatch):
    """the nominal five rounds: frames whose finder latches after four searches skip the fifth launch, their neighbours run it (and
    a sixth or more, which align_batch_finish adds) on caches the first launch wrote"""
    cfg = configs.get("kitti")
    cases = [_case(oracle, "kitti", seed, 600, sigma_t=0.3, sigma_r=0.02) for seed in range(9700, 9712)]  # (poor initial guesses)
    split, searches = _split_and_fused(oracle, monkeypatch, cfg, cases, 512, {}, "mixed")
    assert searches.count(4) >= 3 and sum(n >= 5 for n in searches) >= 3, searches


def test_context_reused_for_other_clouds_and_another_max_fixed(oracle, monkeypatch):
    """one context, four batches: the second has other fixed clouds in the same buffers' shape (nothing of the first may be read),
    the third and fourth another max_fixed and batch size (another stride of both caches)"""
    cfg = configs.get("kitti")
    fkw = dict(search_type=2)
    batches = [([_case(oracle, "kitti", 8400 + b, 800, keep=500 + b) for b in range(5)], 600),
               ([_case(oracle, "kitti", 8500 + b, 800, keep=520 - 7 * b) for b in range(5)], 600),
               ([_case(oracle, "kitti", 8600 + b, 600, keep=300 + 11 * b) for b in range(7)], 384),
               ([_case(oracle, "kitti", 8700 + b, 1500, keep=880 + b) for b in range(3)], 896)]
    ctx = _context(monkeypatch)
    try:
        split = []
        for i, (cases, max_fixed) in enumerate(batches):
            frames = _run_batch(ctx, cfg, cases, max_fixed, fkw, {})
            _against_oracle(oracle, cfg, frames, cases, fkw, "batch %d" % i)
            split.append(_snapshot(frames))
    finally:
        ctx.close()
    ctx = _context(monkeypatch, fused=1)
    try:
        for i, (cases, max_fixed) in enumerate(batches):
            _assert_same(split[i], _snapshot(_run_batch(ctx, cfg, cases, max_fixed, fkw, {})), "batch %d split vs fused" % i)
    finally:
        ctx.close()


def test_captured_graph_replayed_after_the_inputs_were_overwritten_in_place(oracle, monkeypatch):
    """the enqueue sequence captured in a graph, replayed twice on other frames written into the same buffers: the first search of
    every replay rebuilds lattice and rows, nothing of the capture pass or of the previous replay is streamed back"""
    import torch
    cfg = configs.get("kitti")
    fp, ap = _device_params(cfg, {}, {})
    sets = [[_case(oracle, "kitti", 8800 + 50 * s + b, 700, keep=430 + 3 * b + 5 * s) for b in range(6)] for s in range(3)]

    def load(frames, cases):
        frames.reset_state()
        frames.inputs_changed.fill_(1)
        for b, c in enumerate(cases):
            frames.upload(b, c["fixed"], c["dfix"], c["xyz"], c["scale"], c["dmov"], c["X0"])

    ctx = _context(monkeypatch)
    try:
        frames = ops.AlignFrames(0, 6, 512, max(len(c["xyz"]) for cs in sets for c in cs))
        frames.max_fixed = 512
        load(frames, sets[0])
        ops.align_batch(ctx, fp, ap, frames)  # (the scratch buffers exist from here on: nothing is allocated during the capture)
        torch.cuda.synchronize()
        _against_oracle(oracle, cfg, frames, sets[0], {}, "plain call")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            load(frames, sets[0])
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.use_torch_stream()
                ops.align_batch_enqueue(ctx, fp, ap, frames, rounds=5)
            side.synchronize()
            ops.align_batch_finish(ctx)
            got = []
            for s in (1, 2):
                load(frames, sets[s])
                side.synchronize()
                graph.replay()
                ops.align_batch_rearm(ctx)
                ops.align_batch_finish(ctx)
                side.synchronize()
                _against_oracle(oracle, cfg, frames, sets[s], {}, "replay %d" % s)
                got.append(_snapshot(frames))
    finally:
        ctx.close()
    ctx = _context(monkeypatch, fused=1)
    try:
        for s in (1, 2):
            _assert_same(got[s - 1], _snapshot(_run_batch(ctx, cfg, sets[s], 512, {}, {})), "replay %d split vs fused" % s)
    finally:
        ctx.close()


def test_eight_slot_instantiation_tum_shape(oracle, monkeypatch):
    """tum.conf's shape (1024 fixed points, eight survivor slots per thread, depth factor: no mean disparity to bind)"""
    cfg = configs.get("tum")
    cases = [_case(oracle, "tum", 8900 + b, 1100, keep=1024 if b < 2 else None) for b in range(5)]
    cases = [c if len(c["fixed"]) <= 1024 else dict(c, fixed=c["fixed"][:1024], dfix=c["dfix"][:1024]) for c in cases]
    split, searches = _split_and_fused(oracle, monkeypatch, cfg, cases, 1024, {}, "tum")
    assert len(cases[0]["fixed"]) == 1024 and max(len(s["corr"]) for s in split) > 100 and min(searches) >= 2


def test_unpruned_scan_for_the_whole_context(oracle, monkeypatch):
    """PRS_NO_PREFILTER=1: every search takes the unpruned scan, which reads whole rows (both cached half-row arrays)"""
    cfg = configs.get("kitti")
    rng = np.random.default_rng(9001)
    cases = [_case(oracle, "kitti", 9000 + b, 900, keep=560 + b) for b in range(4)] + [_correlated_frame(rng, cfg, 650, corner=False) for _ in range(2)]
    fkw = dict(search_type=2, maximum_search_radius_pixels=100)
    pruned, _ = _split_and_fused(oracle, monkeypatch, cfg, cases, 700, fkw, "pruned")
    unpruned, searches = _split_and_fused(oracle, monkeypatch, cfg, cases, 700, fkw, "unpruned", no_prefilter=1)
    for p, u in zip(pruned, unpruned):
        assert np.array_equal(p["corr"], u["corr"]) and np.array_equal(p["X"], u["X"]) and p["state"] == u["state"] and p["result"] == u["result"]
    assert min(searches) >= 2


def test_mean_disparity_integer_sum_and_float_chain(oracle, monkeypatch):
    """bindFixed's mean disparity, taken by the first search while it builds the lattice: disparities that are whole pixels or
    sixteenths (summed as integers: no addition of the reference's chain can round) and the cases that must take the chain itself
    (one disparity off the 1/16 px grid, sub-pixel right columns, magnitudes that add up to 2^24 sixteenths or more, a single
    disparity of 2^16 px or more).  The mean's bits against the checker's sequential sum, everything else as in the other cases."""
    cfg = configs.get("kitti")
    rng = np.random.default_rng(9100)
    cases = [_case(oracle, "kitti", 9100 + b, 700, keep=440 + b) for b in range(6)]
    n = [len(c["fixed"]) for c in cases]
    cases[1]["fixed"][:, 2] -= rng.integers(0, 16, n[1]).astype(np.float32) / 16.0
    cases[2]["fixed"][n[2] // 2, 2] -= np.float32(1.0 / 32.0)
    cases[3]["fixed"][:, 2] -= rng.uniform(0.0, 1.0, n[3]).astype(np.float32)
    cases[4]["fixed"][:, 2] = cases[4]["fixed"][:, 0] - 2500.0 - (np.arange(n[4]) % 7).astype(np.float32)
    cases[5]["fixed"][3, 2] = cases[5]["fixed"][3, 0] - 70000.0
    sixteenths = [np.abs((c["fixed"][:, 0] - c["fixed"][:, 2]).astype(np.float32) * 16.0) for c in cases]
    on_grid = [bool(np.all(q == np.rint(q))) for q in sixteenths]
    assert on_grid == [True, True, False, False, True, True]
    assert [float(q.sum()) < 2 ** 24 for q in sixteenths] == [True, True, True, True, False, True] and sixteenths[5].max() >= 2 ** 20
    split, _ = _split_and_fused(oracle, monkeypatch, cfg, cases, 512, {}, "disparity")
    for b, c in enumerate(cases):
        assert split[b]["result"][-1] == _bits([oracle.mean_disparity(c["fixed"])]).tolist(), "frame %d: mean disparity bits" % b
