"""The closure merger on the device (csrc/closure_merge.hip) where a real map puts it: 16384 measurements are 256 bitmap words, one
for every thread of the workgroup, so that the scans cross waves, caps end in words of waves 1 to 3 and bin winners sit in all four
(cases: SIZES of tests/closure_merge_cases.py, checked on the CPU by tests/test_closure_merge_ref.py); and the limits the header
states for a call: measurement_stride 16384 / 16385 and the 64 KiB of LDS that the scene bitmap, the measurement bitmaps and the bin
table share.  Every comparison is the one of tests/test_closure_merge_gpu.py: each array of the scene over its whole capacity, the
count and the result byte-identical to the numpy rule.  No tolerance anywhere.

What runs where (test_sizes[...] unless named otherwise):
  the cross-wave half of every scan             every 16384 case: n_cand, pass-1, rest and chosen counts span four waves
  a `before` from another wave                  cap_in_wave_2, from_aligner_inverse_16384 (pass 2), pass1_cut_in_wave_1 (pass 1)
  prefix[] above word 4                         every 16384 case; n_measured_4097 is the first word of wave 1 alone
  a cap inside a word of wave 1 / 2 / 3         pass1_cut_in_wave_1 / cap_in_wave_2 / shared_measurement_16384
  pass-1 winners in all four waves              winners_in_all_waves, xyz_16384, test_two_runs_and_a_replayed_graph_are_byte_identical
  a seen word beyond index 9                    high_landmarks (words 4096 .. 6249, pairs of landmarks 2^16 apart), test_lds_budget
  n_merged from more than five ballots          n_measured_16383 / _16384 (about 3600 merges), test_errors_at_size (11803)
  the limits of a call                          test_stride_16385_is_refused_by_the_batch_entry, test_host_entry_.., test_map_handle_..,
                                                test_lds_budget[1], [0]
  several correspondences on one measurement    shared_measurement, shared_measurement_16384
  bins on exact halves                          half_bins

Single changes of closure_merge.hip that these cases were seen to catch (each built and run once; "old" = tests/test_closure_merge_gpu.py):
  prefix[tid] = the wave-local count            17 fail here (every 16384 case, n_measured_4097, ...); old: 50 pass
  take_first(my_rest, 0, ...)                   15 fail here; old: 15 fail (words of one wave already need `before`)
  take_first(my_rest, wave-local before, ...)   11 fail here (cap_in_wave_2, winners_in_all_waves, xyz_16384, ...); old: 50 pass
  take_first(my_p1, wave-local before, ...)     pass1_cut_in_wave_1 fails; old: 50 pass
  tid < 64 at the my_cand load                  15 fail here; old: 50 pass
  roundf -> rintf in closure_bin                half_bins fails; old: 50 pass
  sh.n_merged added by wave 0 only              9 fail here; old: 30 fail (n_corr_65, n_corr_257 and others reach wave 1)
  seen indexed with s & 0xffff                  high_landmarks fails; old: 50 pass"""
import ctypes as C

import numpy as np
import pytest

import closure_merge_cases as cc
import closure_merge_ref as cr
from srrg2_proslam_amd import _lib
from test_closure_merge_gpu import assert_same, env, params_of, run_batch  # noqa: F401  (env: the module-scoped context fixture)

pytestmark = pytest.mark.gpu
SENTINEL = -77


@pytest.mark.parametrize("name", sorted(cc.SIZES))
def test_sizes(env, name):
    ctx, ops, _ = env
    c = cc.size(name)
    S, r, _ = c["want"]
    (got, res), = run_batch(ctx, ops, [c])
    assert_same(got, res, S, r, name)


def test_mixed_launch_at_stride_16384(env):
    """five workgroups of one launch, from every word in use to none: each pair as it is alone"""
    ctx, ops, _ = env
    cases = cc.mixed_group()
    assert [len(c["measurement"]) for c in cases] == [16384, 4097, 1, 0, 16384] and all(c["P"] == cases[0]["P"] for c in cases)
    for c, (got, res) in zip(cases, run_batch(ctx, ops, cases, stride=16384)):
        S, r, _ = c["want"]
        assert_same(got, res, S, r, c["name"])
        assert r[2] == cr.OK and (r[0] + r[1] > 0 or len(c["measurement"]) == 0)


def test_errors_at_size(env):
    """the sequential walk that settles the code runs over 16000 good entries first; the refused pairs sit beside a good one"""
    ctx, ops, _ = env
    items = cc.error_batch_sizes()
    out = run_batch(ctx, ops, [c for c, _ in items])
    assert [res[2] for _, res in out] == [cr.ERR_DUPLICATE, cr.ERR_RANGE, cr.OK]
    for (c, code), (got, res) in zip(items, out):
        S, r, _ = c["want"]
        assert_same(got, res, S, r, "error %d at size" % code)
        if code != cr.OK:
            assert cr.scenes_equal(got, c["scene"]) and res[:2] == (0, 0)
        else:
            assert res[0] > 256 * 5 and res[1] > 0


# ---- measurement_stride: 16384 is a word for every thread, 16385 is refused at the call ---------------------------------------------
def over_stride():
    return cc.synthetic(seed=92, n_scene=400, n_meas=16385, n_corr=50, target=9000, row_bins=60, col_bins=80)


def test_stride_16385_is_refused_by_the_batch_entry(env):
    ctx, ops, _ = env
    c = over_stride()
    mb = ops.ClosureMergeBatch(0, 1, c["scene"]["coords"].shape[0], 16385, 64)
    mb.upload(0, c["scene"], c["measurement"], c["measurement_desc"], c["corr"], c["transform"], c["scene_in_world"])
    mb.result.fill_(SENTINEL)
    with pytest.raises(_lib.ProslamHipError) as e:
        ops.closure_merge_batch(ctx, params_of(c["P"]), mb)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    ctx.synchronize()
    assert mb.result_of(0) == (SENTINEL,) * 3 and cr.scenes_equal(mb.scene_of(0), c["scene"])
    # one measurement fewer in the same arrays is the accepted limit
    mb.measurement_stride = 16384  # (the rows of a single pair do not depend on the stride)
    mb.n_measured[0] = 16384
    ops.closure_merge_batch(ctx, params_of(c["P"]), mb)
    ctx.synchronize()
    S, r, _ = cc.want(dict(c, measurement=c["measurement"][:16384], measurement_desc=c["measurement_desc"][:16384]))
    assert_same(mb.scene_of(0), mb.result_of(0), S, r, "stride 16384")


def test_host_entry_at_16384_and_16385(env):
    ctx, ops, _ = env
    c = cc.size("winners_in_all_waves")
    S, r, _ = c["want"]
    got, res = ops.closure_merge(ctx, params_of(c["P"]), c["scene"], c["measurement"], c["measurement_desc"], c["corr"], c["transform"],
                                 c["scene_in_world"])
    assert_same(got, res, S, r, "host entry, 16384")
    # 16385: the header's limit, PRS_ERR_UNSUPPORTED, and the caller's arrays as they were
    c = over_stride()
    mine = cr.copy_scene(c["scene"])
    n, out = C.c_int32(mine["n_points"]), (C.c_int32 * 3)(SENTINEL, SENTINEL, SENTINEL)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    z, d, corr, T, W = (np.ascontiguousarray(c[k]) for k in ("measurement", "measurement_desc", "corr", "transform", "scene_in_world"))
    P = params_of(c["P"])
    rc = _lib.load().prs_closure_merge(ctx._h, C.byref(P), len(mine["coords"]), C.byref(n), p(mine["coords"]), p(mine["desc"]), p(mine["state"]),
                                       p(mine["covariance"]), p(mine["n_opt"]), p(mine["inlier"]), p(mine["n_meas"]), p(W), p(z), p(d), 16385,
                                       p(corr), len(corr), 0, p(T), 0, out)
    assert rc == _lib.ERR_UNSUPPORTED
    mine["n_points"] = n.value
    assert cr.scenes_equal(mine, c["scene"]) and tuple(out) == (SENTINEL,) * 3


def plain_scene(c):
    """what MapHandle.set_scene makes of a case's cloud: state = coordinates, every other statistic zero"""
    n = c["scene"]["n_points"]
    return cr.make_scene(c["scene"]["coords"].shape[0], c["scene"]["coords"][:n, :3], c["scene"]["desc"][:n])


def handle_scene_equals(m, S):
    got, k = m.scene(), S["n_points"]
    assert m.size()[0] == k == len(got["coords"])
    for name in ("coords", "state"):
        assert np.array_equal(got[name].view(np.uint32), S[name][:k, :3].view(np.uint32)), name
    for name in ("desc", "n_opt", "inlier"):
        assert np.array_equal(got[name], S[name][:k]), name


def test_map_handle_at_16384_and_16385(env):
    ctx, ops, _ = env
    c = cc.size("winners_in_all_waves")
    plain = dict(c, scene=plain_scene(c), scene_in_world=np.eye(4, dtype=np.float32))
    S, r, _ = cc.want(plain)
    (got, res), = run_batch(ctx, ops, [plain])
    assert_same(got, res, S, r, "batch entry on the handle's scene")
    n, cap = plain["scene"]["n_points"], len(plain["scene"]["coords"])
    m = ops.MapHandle(ctx, cap, max_measured=16384)
    m.set_scene(plain["scene"]["coords"][:n, :3], plain["scene"]["desc"][:n])
    assert m.merge_closure(params_of(c["P"]), c["transform"], c["measurement"], c["measurement_desc"], c["corr"]) == r
    handle_scene_equals(m, S)
    # one measurement more than the handle was made for: PRS_ERR_CAPACITY, the map as it was
    big = over_stride()
    with pytest.raises(_lib.ProslamHipError) as e:
        m.merge_closure(params_of(big["P"]), big["transform"], big["measurement"], big["measurement_desc"], big["corr"])
    assert e.value.status == _lib.ERR_CAPACITY
    handle_scene_equals(m, S)
    m.close()
    # a handle made for 16385 measurements: its stride is beyond the limit, the call says so and the map stays as it was
    c = over_stride()
    before = plain_scene(c)
    m = ops.MapHandle(ctx, len(before["coords"]), max_measured=16385)
    m.set_scene(before["coords"][:400, :3], before["desc"][:400])
    with pytest.raises(_lib.ProslamHipError) as e:
        m.merge_closure(params_of(c["P"]), c["transform"], c["measurement"], c["measurement_desc"], c["corr"])
    assert e.value.status == _lib.ERR_UNSUPPORTED
    handle_scene_equals(m, before)
    m.close()


# ---- the LDS budget: capacity / 8 + 36 bytes per word of the measurement bitmaps + 8 bytes per bin share 64 KiB ----------------------
def largest_capacity(ctx, ops, mb, P):
    """the largest capacity (a multiple of 32) the batch entry accepts for mb's stride and P's bins, by bisection on the return
    code; every probe is an empty pair (0 landmarks, 0 measurements, 0 correspondences) in arrays allocated for the upper end"""
    upper = mb.capacity
    mb.n_points.zero_(), mb.n_measured.zero_(), mb.n_corr.zero_()

    def accepted(cap):
        mb.capacity = cap
        mb.result.fill_(SENTINEL)
        try:
            ops.closure_merge_batch(ctx, P, mb)
        except _lib.ProslamHipError as e:
            assert e.status == _lib.ERR_UNSUPPORTED
            ctx.synchronize()
            assert mb.result_of(0) == (SENTINEL,) * 3  # nothing launched
            return False
        ctx.synchronize()
        assert mb.result_of(0) == (0, 0, cr.OK)
        return True

    lo, hi = 1, upper // 32  # in units of 32 landmarks: lo accepted, hi refused
    assert accepted(32 * lo) and not accepted(32 * hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(32 * mid) else (lo, mid)
    mb.capacity = upper
    return 32 * lo


@pytest.mark.parametrize("binning", [1, 0])
def test_lds_budget(env, binning):
    """with 60 x 80 bins the three tables share the 64 KiB; without binning the scene bitmap has them almost alone"""
    ctx, ops, _ = env
    args = dict(cc.SIZES["winners_in_all_waves"][0], binning=binning, with_stats=bool(binning), target=9000 if binning else 100000)
    P = params_of(cc.synthetic(**dict(args, n_meas=1, n_corr=0))["P"])
    probe = ops.ClosureMergeBatch(0, 1, 1 << 19, 16384, 64, with_stats=False)
    best = largest_capacity(ctx, ops, probe, P)
    del probe
    # the header's limits paragraph, with 1 KiB of room for the kernel's fixed part: a condition, not a measurement
    used = best // 8 + 36 * 256 + (8 * 62 * 82 if binning else 0)
    print("largest capacity %d: %d bytes of bitmaps and bins" % (best, used))
    assert 65536 - 1024 <= used <= 65536, (best, used)
    # at the limit the launch asks for the whole 64 KiB; the landmarks named lie in the last 64 rows, the bitmap's last words
    n_scene = best - 16384
    c = cc.synthetic(**dict(args, n_scene=n_scene, capacity=best, landmarks_from=n_scene - 64))
    S, r, info = cc.want(c)
    assert r[2] == cr.OK and r[0] > 25 and cc.per_wave(info["added"]).all() and S["n_points"] <= best, r
    assert cc.merged_landmarks(info, c).min() >= n_scene - 64
    (got, res), = run_batch(ctx, ops, [c])
    assert_same(got, res, S, r, "capacity %d" % best)
    # 32 landmarks more: refused at the call, nothing written
    over = cc.synthetic(**dict(args, n_scene=n_scene, capacity=best + 32, landmarks_from=n_scene - 64))
    mb = ops.ClosureMergeBatch(0, 1, best + 32, 16384, 64, with_stats=bool(binning))
    mb.upload(0, over["scene"], over["measurement"], over["measurement_desc"], over["corr"], over["transform"], over["scene_in_world"])
    mb.result.fill_(SENTINEL)
    with pytest.raises(_lib.ProslamHipError) as e:
        ops.closure_merge_batch(ctx, P, mb)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    ctx.synchronize()
    assert mb.result_of(0) == (SENTINEL,) * 3 and cr.scenes_equal(mb.scene_of(0), over["scene"])


# ---- the bin winners go through LDS atomicMin: the order of arrival must not show ---------------------------------------------------
def test_two_runs_and_a_replayed_graph_are_byte_identical(env):
    import torch
    ctx, ops, _ = env
    c = cc.size("winners_in_all_waves")
    S, r, _ = c["want"]
    (a, ra), = run_batch(ctx, ops, [c])
    (b, rb), = run_batch(ctx, ops, [c])
    assert ra == rb and cr.scenes_equal(a, b)
    assert_same(a, ra, S, r, "first run")
    mb = ops.ClosureMergeBatch(0, 1, len(c["scene"]["coords"]), 16384, len(c["corr"]))
    up = lambda: mb.upload(0, c["scene"], c["measurement"], c["measurement_desc"], c["corr"], c["transform"], c["scene_in_world"])  # noqa: E731
    up()
    P = params_of(c["P"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        ops.closure_merge_batch(ctx, P, mb)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ops.closure_merge_batch(ctx, P, mb)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    for what in ("replay", "second replay"):
        up()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = mb.scene_of(0)
        assert_same(got, mb.result_of(0), S, r, what)
        assert cr.scenes_equal(got, a)
