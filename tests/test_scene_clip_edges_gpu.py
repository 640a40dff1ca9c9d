"""The scene clipper's kernels (csrc/scene_clip.hip) on the cases of tests/scene_clip_cases.py, in each of its launch shapes:
the walk (one workgroup per scene, a running offset from tile to tile) with one, two, four and five tiles, count + scatter, and
the single scene of the host entry.  The expectation is scene_clip_ref.clip: coordinates as uint32 bit patterns, descriptors,
indices, counts and statuses equal.  tests/test_scene_clip_cases.py shows on the CPU what each case holds.

Every launch starts from output buffers filled with a sentinel byte, and one scene more is allocated than is launched: what lies
at and past n_clipped of a scene, the whole of an empty scene with its n_clipped, and the scene behind the last one keep it."""
import ctypes as C

import numpy as np
import pytest

import scene_clip_cases as cc
import scene_clip_ref as ref
from srrg2_proslam_amd import _lib, ops

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A
SENTINEL32 = int.from_bytes(bytes([SENTINEL] * 4), "little")
I4 = cc.I4


def shape_of(B, stride):
    """the launcher's choice (scene_clip_launch): 'walk' for many scenes or at most two tiles, else 'count+scatter'"""
    return "walk" if B >= 128 or -(-stride // cc.TILE) <= 2 else "count+scatter"


def load(batch, with_nopt=False):
    """the batch in device memory, one unlaunched scene behind it"""
    import torch
    B, stride = len(batch["n_scene"]), batch["stride"]
    sc = ops.ClipScenes(0, B + 1, stride)
    sc.batch = B
    put(sc, batch)
    if with_nopt:
        sc.scene_n_opt = torch.zeros((B + 1, stride), dtype=torch.int32, device=sc.scene_xyzw.device)
        sc.scene_n_opt[:B] = torch.from_numpy(batch["n_opt"].view(np.int32)).to(sc.scene_xyzw.device)
    return sc


def put(sc, batch):
    import torch
    B, dev = sc.batch, sc.scene_xyzw.device
    sc.scene_xyzw[:B] = torch.from_numpy(batch["xyzw"]).to(dev)
    sc.scene_desc[:B] = torch.from_numpy(batch["desc"]).to(dev)
    sc.n_scene[:B] = torch.from_numpy(batch["n_scene"]).to(dev)
    sc.robot_in_local_map[:B] = torch.from_numpy(batch["R"]).to(dev)


def outputs(sc):
    return (sc.clipped_xyzw, sc.clipped_desc, sc.global_indices, sc.n_clipped, sc.status)


def fill(sc):
    import torch
    for t in outputs(sc):
        t.view(torch.uint8).fill_(SENTINEL)


def download(sc):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outputs(sc)]


def launch(ctx, sc, batch):
    fill(sc)
    ops.scene_clip_batch(ctx, cc.projector(_lib, batch["proj"]), batch["S"], sc)
    ctx.synchronize()
    return download(sc)


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENTINEL).all())


def check(out, batch, with_nopt=False):
    """every scene against scene_clip_ref.clip, and everything the kernels must not write"""
    xyzw, desc, idx, count, status = out
    B = len(batch["n_scene"])
    for b in range(B):
        what = "%s scene %d (%s, n_scene %d)" % (batch["key"], b, batch["names"][b], batch["n_scene"][b])
        wx, wd, wi, m, st = cc.expected(batch, b, with_nopt)
        assert int(status[b]) == st, what
        if st == ref.WARN_EMPTY_INPUT:  # nothing is written, the count included
            assert int(count[b]) == SENTINEL32, what
            m = 0
        else:
            assert int(count[b]) == m, what
        assert np.array_equal(idx[b, :m], wi), what
        assert np.array_equal(ref.bits(xyzw[b, :m]), ref.bits(wx)), what
        assert np.array_equal(desc[b, :m], wd), what
        assert untouched(xyzw[b, m:]) and untouched(desc[b, m:]) and untouched(idx[b, m:]), what
    assert all(untouched(a[B:]) for a in out), "the scene behind the last one"


def same_bytes(a, b, scenes):
    for x, y in zip(a, b):
        assert np.array_equal(np.ascontiguousarray(x[:scenes]).view(np.uint8), np.ascontiguousarray(y[:scenes]).view(np.uint8))


@pytest.fixture(scope="module")
def walked(hip_ctx):
    """the two ragged batches through the walk (four and five tiles), once for the module: -> {(B, stride): outputs}"""
    done = {}
    for B, stride in ((128, 3073), (130, 4097)):
        batch = cc.ragged(B, stride)
        assert shape_of(B, stride) == "walk" and -(-stride // cc.TILE) >= 3
        sc = load(batch)
        done[(B, stride)] = launch(hip_ctx, sc, batch)
        del sc
    return done


@pytest.mark.parametrize("shape", [(128, 3073), (130, 4097)], ids=["128x3073", "130x4097"])
def test_walk_with_four_and_five_tiles(walked, shape):
    check(walked[shape], cc.ragged(*shape))


@pytest.mark.parametrize("shape", [(128, 3073), (130, 4097)], ids=["128x3073", "130x4097"])
def test_count_and_scatter_on_the_first_127_scenes_agrees_with_the_walk(hip_ctx, walked, shape):
    batch = cc.head(cc.ragged(*shape), 127)
    assert shape_of(127, batch["stride"]) == "count+scatter"
    out = launch(hip_ctx, load(batch), batch)
    check(out, batch)
    same_bytes(out, walked[shape], 127)


@pytest.mark.parametrize("shape", [(128, 3073), (130, 4097)], ids=["128x3073", "130x4097"])
def test_scene_alone_equals_the_scene_in_its_batch(hip_ctx, walked, shape):
    batch = cc.ragged(*shape)
    xyzw, desc, idx, count, _ = walked[shape]
    pg = cc.projector(_lib, batch["proj"])
    names = batch["names"]
    picked = [names.index("edges"), names.index("pattern:alt_wave"), names.index("inside_tail"), names.index("n=1025"), len(names) - 1]
    for b in picked:
        n, m = cc.rows_of(batch, b), int(count[b])
        got = ops.scene_clip(hip_ctx, pg, batch["R"][b], batch["S"], batch["xyzw"][b, :n], batch["desc"][b, :n])
        assert np.array_equal(got[0].view(np.uint8), xyzw[b, :m].view(np.uint8)) and np.array_equal(got[1], desc[b, :m]), names[b]
        assert np.array_equal(got[2], idx[b, :m]) and got[3] == cc.expected(batch, b)[4], names[b]


@pytest.mark.parametrize("stride", [700, 1024, 1025, 2048, 2049])
@pytest.mark.parametrize("with_nopt", [False, True], ids=["w", "ages"])
def test_one_two_and_three_tiles(hip_ctx, stride, with_nopt):
    """three scenes: the walk up to stride 2048, count + scatter at 2049; with and without the age column"""
    batch = cc.small(stride)
    assert shape_of(3, stride) == ("walk" if stride <= 2048 else "count+scatter")
    check(launch(hip_ctx, load(batch, with_nopt), batch), batch, with_nopt)


@pytest.mark.parametrize("shape,count", [((128, 3073), 128), ((128, 3073), 127)], ids=["walk", "count+scatter"])
def test_ages_in_both_launch_shapes(hip_ctx, shape, count):
    batch = cc.head(cc.ragged(*shape), count)
    assert shape_of(count, batch["stride"]) == ("walk" if count == 128 else "count+scatter")
    out = launch(hip_ctx, load(batch, True), batch)
    check(out, batch, True)
    # the w column comes from the ages of the SOURCE rows, the scene's own w is ignored
    b = batch["names"].index("pattern:alt_row")
    m = int(out[3][b])
    want = ops.info_scale_from_nopt(np.minimum(batch["n_opt"][b][out[2][b, :m]], np.uint32(4095)))
    assert m > 1000 and np.array_equal(out[0][b, :m, 3].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("n", cc.SIZES)
def test_keep_patterns(hip_ctx, n):
    """the eight patterns as one batch at stride n: the walk up to 2048 rows, count + scatter above"""
    batch = cc.blank("patterns-%d" % n, len(cc.PATTERNS), n, "planted", I4)
    want = []
    for b, kind in enumerate(cc.PATTERNS):
        xyzw, desc, idx = cc.pattern_scene(kind, n, b)
        cc.put_scene(batch, b, "pattern:" + kind, xyzw, desc)
        want.append(idx)
    xyzw, desc, idx, count, status = launch(hip_ctx, load(batch), batch)
    for b, kind in enumerate(cc.PATTERNS):
        m = len(want[b])
        assert int(count[b]) == m and int(status[b]) == (ref.OK if m else ref.WARN_NO_PROJECTION), (kind, n)
        assert np.array_equal(idx[b, :m], want[b]), (kind, n)  # the closed form
        assert np.array_equal(xyzw[b, :m, 3], cc.signature_w(want[b])) and np.array_equal(desc[b, :m], cc.signature_desc(want[b], b)), (kind, n)
        assert np.array_equal(xyzw[b, :m, :3].view(np.uint32), np.tile(cc.INSIDE_POINT, (m, 1)).view(np.uint32)), (kind, n)
        assert untouched(xyzw[b, m:]) and untouched(desc[b, m:]) and untouched(idx[b, m:]), (kind, n)
    assert all(untouched(a[len(cc.PATTERNS):]) for a in (xyzw, desc, idx, count, status))


@pytest.mark.parametrize("name", ["planted", "tall"])
def test_frustum_edges_through_the_host_entry(hip_ctx, name):
    """the planted cloud alone (1300 rows, two tiles: the walk): every verdict is the one stated where the point was planted"""
    c = cc.edge_cloud(name)
    got = ops.scene_clip(hip_ctx, cc.projector(_lib, name), I4, I4, c["xyzw"], c["desc"])
    assert np.array_equal(got[2], np.flatnonzero(c["keep"]))
    want = ref.clip(cc.plain(name), I4, I4, c["xyzw"], c["desc"])
    assert np.array_equal(ref.bits(got[0]), ref.bits(want[0])) and np.array_equal(got[1], want[1]) and got[3] == want[4]
    P = cc.planted(name)
    kept = np.isin(c["planted_rows"], got[2])
    assert np.array_equal(kept, ref.inside(cc.plain(name), P["xyz"][c["planted_index"]]))  # the float64 statement


@pytest.mark.parametrize("name", list(cc.sensor_offsets()))
def test_sensor_offsets(hip_ctx, name):
    S, _ = cc.sensor_offsets()[name]
    xyzw, desc, R = cc.sensor_scene()
    got = ops.scene_clip(hip_ctx, cc.projector(_lib, "planted"), R, S, xyzw, desc)
    want = ref.clip(cc.plain("planted"), R, S, xyzw, desc)
    assert np.array_equal(got[2], want[2]) and np.array_equal(ref.bits(got[0]), ref.bits(want[0])) and np.array_equal(got[1], want[1])


def test_captured_graph_replays_the_walk(hip_ctx):
    import torch
    ctx = hip_ctx
    first, second = cc.ragged(128, 3073), cc.ragged(130, 4097)
    # the replay runs on other scenes written into the same buffers: the first 128 of the five-tile batch cut to the stride
    other = cc.blank("replay", 128, 3073, "planted", I4)
    for key in ("xyzw", "desc", "n_opt"):
        other[key] = np.ascontiguousarray(second[key][:128, :3073])
    other["n_scene"], other["R"], other["names"] = np.minimum(second["n_scene"][:128], 3073), second["R"][:128], second["names"][:128]
    sc = load(first)
    pg = cc.projector(_lib, "planted")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        ops.scene_clip_batch(ctx, pg, I4, sc)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ops.scene_clip_batch(ctx, pg, I4, sc)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    put(sc, other)
    fill(sc)
    torch.cuda.synchronize()
    g.replay()
    check(download(sc), other)


def test_host_entry_capacity_and_carried_w(hip_ctx):
    L = _lib.load()
    xyzw, desc, idx = cc.pattern_scene("alt_row", 1025)
    n = len(xyzw)
    pg = cc.projector(_lib, "planted")
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for capacity, rc in ((n, ref.OK), (n - 1, _lib.ERR_CAPACITY)):
        out_xyzw = np.full((n, 4), np.float32(-5.0))
        out_desc = np.full((n, 32), SENTINEL, np.uint8)
        out_idx = np.full(n, -5, np.int32)
        m = C.c_int32(-5)
        assert L.prs_scene_clip(hip_ctx._h, C.byref(pg), p(I4), p(I4), p(xyzw), p(desc), n, p(out_xyzw), p(out_desc), p(out_idx),
                                capacity, C.byref(m)) == rc
        if rc == ref.OK:
            k = m.value
            assert k == len(idx) and np.array_equal(out_idx[:k], idx) and np.array_equal(out_desc[:k], desc[idx])
            assert np.array_equal(out_xyzw[:k, 3], cc.signature_w(idx))  # this entry takes no ages: w is carried through
            assert (out_xyzw[k:] == -5.0).all() and (out_idx[k:] == -5).all() and untouched(out_desc[k:])
        else:
            assert b"capacity" in L.prs_last_error(hip_ctx._h)
            assert m.value == -5 and (out_xyzw == -5.0).all() and (out_idx == -5).all() and untouched(out_desc)
