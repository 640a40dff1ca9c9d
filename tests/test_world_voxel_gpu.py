"""The world voxel filter on the device (ops.WorldVoxelBatch: prs_world_voxel_batch_run) against its numpy restatement
(tests/world_voxel_ref.py).  Every output array is compared byte for byte: both sides do the same IEEE operations and the same integer
sums, so no tolerance is involved.  Output rows the call must not touch are checked against a sentinel."""
import ctypes as C

import numpy as np
import pytest

import world_voxel_cases as vc
import world_voxel_ref as ref
from srrg2_proslam_amd import _lib, ops

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0xA5
INPUTS = ops.WorldVoxelBatch.INPUTS
ROW_OUTPUTS = ("xyz",) + ops.WorldVoxelBatch.OPTIONAL
COUNTS = ("n_out", "n_voxels", "n_nonfinite", "n_outside", "status")
POSITIONS = ("representative", "mean")
# 0.3 is not a float32 and no coordinate is a multiple of it; EDGE_SIZE (0.5) is exact, for rows planted on faces and edges
SIZE = 0.3


def expected_of(clouds, inputs, p, out_stride, table_stride):
    """the restatement's result for every cloud of a list, given the optional input arrays `inputs`.  out_stride None: the
    count-only call.  Runs on the host alone"""
    rp = ref.params(p.voxel_size, p.position)
    clouds = [dict(c, **{k: None for k in INPUTS if k not in inputs}) for c in clouds]
    return [ref.world_voxel(c, rp, out_stride, table_stride) for c in clouds]


class Rig:
    """a WorldVoxelBatch over device copies of a list of clouds in the restatement's layout.  inputs: which of the optional input
    arrays the call is given (the others are not uploaded).  known: results of expected_of for these clouds, out_stride and
    table_stride that a test formed before it built the rig, {(position, count_only): results}; they are not computed again"""

    def __init__(self, ctx, clouds, out_stride, table_stride=None, outputs=ops.WorldVoxelBatch.OPTIONAL, inputs=INPUTS, known=None):
        import torch
        self.ctx, self.clouds, self.B, self.inputs, self.known = ctx, clouds, len(clouds), tuple(inputs), dict(known or {})
        N = clouds[0]["in_stride"]
        dev = torch.device("cuda", 0)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.dev = dict(xyz=z((self.B, N, 4), torch.float32), n_out=z((self.B,), torch.int32))
        for k in self.inputs:
            self.dev[k] = z((self.B, N, 32), torch.uint8) if k == "desc" else z((self.B, N), torch.int32)
        self.vx = ops.WorldVoxelBatch(self.B, N, out_stride, table_stride, outputs)
        self.upload()

    def cloud(self):
        return dict(self.dev)

    def upload(self):
        import torch
        for k, t in self.dev.items():
            a = np.stack([np.asarray(c["n"] if k == "n_out" else c[k]) for c in self.clouds])
            a = np.ascontiguousarray(a.astype(np.int32) if k == "n_out" else a)
            t.copy_(torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).reshape(t.shape))

    def fill_sentinel(self):
        import torch
        for k in ROW_OUTPUTS + COUNTS:
            t = self.vx.tensor(k)
            if t is not None:
                t.view(torch.uint8).fill_(SENTINEL)

    def outputs(self):
        return {k: self.vx.tensor(k).cpu().numpy() for k in ROW_OUTPUTS + COUNTS if self.vx.tensor(k) is not None}

    def expected(self, p, count_only=False):
        if (p.position, count_only) in self.known:
            return self.known[p.position, count_only]
        return expected_of(self.clouds, self.inputs, p, None if count_only else self.vx.out_stride, self.vx.table_stride)

    def compare(self, got, want, what=""):
        for b, w in enumerate(want):
            tag = (what, b)
            for k in COUNTS:
                assert int(got[k][b]) == w[k], tag + (k, int(got[k][b]), w[k])
            n = w["n_out"]
            for k in ROW_OUTPUTS:
                if k not in got:
                    continue
                if k in INPUTS and k not in self.inputs:
                    n_k = 0  # gathered only when both the input and the output are set
                else:
                    n_k = n
                    assert got[k][b, :n].tobytes() == np.ascontiguousarray(w[k]).tobytes(), tag + (k,)
                assert (got[k][b, n_k:].view(np.uint8) == SENTINEL).all(), tag + (k, "rows behind n_out")

    def check(self, p, count_only=False, what=""):
        """run (or count) and compare every sequence with the restatement; -> the restatement's results"""
        self.upload()
        self.fill_sentinel()
        (self.vx.count if count_only else self.vx.run)(self.ctx, p, self.cloud())
        self.ctx.synchronize()
        want = self.expected(p, count_only)
        self.compare(self.outputs(), want, what)
        return want

    def check_both(self, size, what="", count_only=False):
        return [self.check(ops.world_voxel_params(size, position), count_only, what + " " + position) for position in POSITIONS]


def _rng(*seed):
    return np.random.default_rng(list(seed))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 2305])
def test_rows_and_chunks(hip_ctx, n):
    """in_n up to ten chunks of 256 rows, in an array a little longer than that; about four rows to a voxel, interleaved"""
    c = vc.make_cloud(_rng(1, n), n + 3, n, SIZE, max(n // 4, 1))
    rig = Rig(hip_ctx, [c], n + 3)
    for want in rig.check_both(SIZE, "n %d" % n):
        assert want[0]["status"] == ref.PRS_OK and want[0]["n_voxels"] == (max(n // 4, 1) if n else 0)
        assert want[0]["count"].sum() == n
    rig.check_both(SIZE, "count only", count_only=True)


def test_every_row_in_its_own_voxel(hip_ctx):
    c = vc.make_cloud(_rng(2), 2305, 2305, SIZE, 2305)
    rig = Rig(hip_ctx, [c], 2305)
    for want in rig.check_both(SIZE):
        assert want[0]["n_voxels"] == 2305 and want[0]["index"].tolist() == list(range(2305))


def test_all_rows_in_one_voxel(hip_ctx):
    """the worst contention: 2305 compare-and-swaps, mins and adds on one slot, and the MEAN of all of them"""
    c = vc.one_voxel_cloud(_rng(3), 2305, 2305, SIZE)
    c["n_opt"][1234], c["n_opt"][2000] = 9, 9  # the representative sits in the middle of a chunk, the tie goes to the lower row
    rig = Rig(hip_ctx, [c], 5)
    for want in rig.check_both(SIZE):
        assert want[0]["n_voxels"] == 1 and want[0]["index"].tolist() == [1234] and want[0]["count"].tolist() == [2305]


@pytest.mark.parametrize("voxels", [4, 64])
def test_a_full_table_and_one_voxel_more(hip_ctx, voxels):
    """table_stride equal to the number of voxels: every slot taken, probes wrap past the end; one voxel more overflows"""
    c = vc.make_cloud(_rng(4, voxels), 300, 257, SIZE, voxels)
    rig = Rig(hip_ctx, [c], 300, table_stride=voxels)
    for want in rig.check_both(SIZE, "full"):
        assert want[0]["status"] == ref.PRS_OK and want[0]["n_voxels"] == voxels
    c["xyz"][256, :3] = F(1000.0)  # the last row, alone in a voxel far from the others
    for want in rig.check_both(SIZE, "one more"):
        assert (want[0]["status"], want[0]["n_out"], want[0]["n_voxels"]) == (ref.PRS_ERR_CAPACITY, 0, -1)
    rig.check_both(SIZE, "one more, count only", count_only=True)
    c["n"] = 256  # without that row the table is full again: nothing of the overflow is left behind
    for want in rig.check_both(SIZE, "full again"):
        assert want[0]["status"] == ref.PRS_OK and want[0]["n_voxels"] == voxels


def test_table_of_one_slot(hip_ctx):
    c = vc.one_voxel_cloud(_rng(5), 70, 65, SIZE)
    rig = Rig(hip_ctx, [c], 70, table_stride=1)
    assert all(w[0]["n_voxels"] == 1 for w in rig.check_both(SIZE))
    c["xyz"][64, 0] += F(5.0)
    assert all(w[0]["n_voxels"] == -1 for w in rig.check_both(SIZE))


def test_truncation_and_count_only(hip_ctx):
    c = vc.make_cloud(_rng(6), 600, 515, SIZE, 130)
    rig = Rig(hip_ctx, [c], 600)
    counted = rig.check_both(SIZE, count_only=True)  # sizes the output: nothing but the counts and the status is written
    assert all(w[0]["n_voxels"] == 130 and w[0]["n_out"] == 0 and w[0]["status"] == ref.PRS_OK for w in counted)
    for out_stride, status in ((130, ref.PRS_OK), (129, ref.PRS_ERR_CAPACITY), (1, ref.PRS_ERR_CAPACITY)):
        rig = Rig(hip_ctx, [c], out_stride)
        for want in rig.check_both(SIZE, "out_stride %d" % out_stride):
            assert (want[0]["status"], want[0]["n_out"], want[0]["n_voxels"]) == (status, min(130, out_stride), 130)


def test_optional_inputs_and_outputs(hip_ctx):
    c = vc.make_cloud(_rng(7), 300, 257, SIZE, 60)
    with_n_opt = Rig(hip_ctx, [c], 300).check_both(SIZE)
    rig = Rig(hip_ctx, [c], 300, inputs=("desc", "node", "row"))  # in_n_opt NULL: every row has n_opt 0, the lowest row represents
    assert not rig.vx.descriptor(rig.cloud()).in_n_opt
    for want, other in zip(rig.check_both(SIZE, "no n_opt"), with_n_opt):
        assert "n_opt" not in want[0] and want[0]["index"].tolist() != other[0]["index"].tolist()
    Rig(hip_ctx, [c], 300, inputs=()).check_both(SIZE, "no optional input")
    for absent in ops.WorldVoxelBatch.OPTIONAL:
        keep = tuple(k for k in ops.WorldVoxelBatch.OPTIONAL if k != absent)
        rig = Rig(hip_ctx, [c], 300, outputs=keep)
        assert rig.vx.tensor(absent) is None and not getattr(rig.vx.descriptor(rig.cloud()), absent)
        rig.check_both(SIZE, "without " + absent)
    rig = Rig(hip_ctx, [c], 300, outputs=())
    rig.check_both(SIZE, "xyz alone")
    cloud = rig.vx.cloud_of(0)
    assert sorted(cloud) == ["bounds", "n_nonfinite", "n_out", "n_outside", "n_total", "n_voxels", "status", "xyz"]


def test_edges_at_the_ends_of_waves_and_chunks(hip_ctx):
    """negative, face-exact, -0.0, non-finite and outside-the-grid coordinates at the first and last lane of waves and chunks"""
    s = vc.EDGE_SIZE
    c = vc.make_cloud(_rng(8), 2305, 2305, s, 400)
    at = [0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 254, 255, 256, 257, 319, 320, 511, 512, 767, 768, 1023, 1024, 2047, 2048, 2111, 2112,
          2302, 2303, 2304]
    planted = vc.plant_edges(c, at) + vc.plant_edges(c, [r + 700 for r in at[:len(vc.EDGES)]][::-1])
    rig = Rig(hip_ctx, [c], 2305)
    for want in rig.check_both(s):
        w = want[0]
        assert w["n_nonfinite"] == sum(f == "nonfinite" for _, _, f in planted) >= 6
        assert w["n_outside"] == sum(f == "outside" for _, _, f in planted) >= 6
        assert w["count"].sum() == 2305 - w["n_nonfinite"] - w["n_outside"]
    # a wave and a chunk whose rows are all dropped
    c["xyz"][64:128, 0] = F(np.nan)
    c["xyz"][1024:1280, 2] = F(-1e9)
    for want in rig.check_both(s, "a whole wave, a whole chunk"):
        assert want[0]["n_nonfinite"] >= 64 and want[0]["n_outside"] >= 256


def _three(seed):
    """B = 3 with in_n of 0, 2305 and in_stride + 1"""
    N = 2310
    clouds = [vc.make_cloud(_rng(seed, b), N, n, SIZE, 500) for b, n in enumerate((0, 2305, N + 1))]
    return clouds


def test_a_refused_sequence_behind_its_neighbours(hip_ctx):
    rig = Rig(hip_ctx, _three(9), 600)
    for want in rig.check_both(SIZE):  # the sentinel in everything the refused sequence owns is compared in check()
        assert [w["status"] for w in want] == [ref.PRS_OK, ref.PRS_OK, ref.PRS_ERR_RANGE]
        assert [w["n_voxels"] for w in want] == [0, 500, 0]
    rig.check_both(SIZE, "count only", count_only=True)


def test_a_refused_sequence_between_its_neighbours(hip_ctx):
    """a negative in_n between a sequence that is truncated and a short one"""
    clouds = [vc.make_cloud(_rng(9, 3 + b), 2310, n, SIZE, 700) for b, n in enumerate((2310, -1, 257))]
    rig = Rig(hip_ctx, clouds, 600)
    for want in rig.check_both(SIZE):
        assert [w["status"] for w in want] == [ref.PRS_ERR_CAPACITY, ref.PRS_ERR_RANGE, ref.PRS_OK]
        assert [w["n_voxels"] for w in want] == [700, 0, 257]
    rig.check_both(SIZE, "count only", count_only=True)


def _snapshot(rig, b):
    return {k: v[b].tobytes() for k, v in rig.outputs().items()}


@pytest.mark.parametrize("position", POSITIONS)
def test_a_sequence_does_not_depend_on_its_batch_or_on_the_run(hip_ctx, position):
    clouds = _three(10)[::-1]  # the refused one first, the full one in the middle
    clouds[2] = vc.make_cloud(_rng(10, 7), 2310, 2305, SIZE, 300)
    p = ops.world_voxel_params(SIZE, position)
    rig3 = Rig(hip_ctx, clouds, 400)
    rig3.check(p)
    first = _snapshot(rig3, 2)
    rig3.check(p)
    assert _snapshot(rig3, 2) == first  # two runs
    rig1 = Rig(hip_ctx, [clouds[2]], 400)
    rig1.check(p)
    assert _snapshot(rig1, 0) == first  # position 0 of B = 1 against position 2 of B = 3


# ---- beyond one wave and one tile of the scan.  The scan kernel runs roundup64(ceil(chunks / 8)) threads, at most 1024, over tiles of
# 8 * threads chunks: 512 chunks are the last single wave, 513 take two; 8192 chunks are one tile of 1024 threads, 8193 start a second
# one, whose bases stand on the carry.  voxels: more than 2^16 and 2^20, so that chunk bases pass both
BIG_VOXELS = {131072: 80000, 131073: 80000, 2097152: 1200000, 2097153: 1200000}
BIG_SIDE = 200  # 8e6 cells: room for 1.2 million voxels


def _big_cloud(rows):
    """in_n = in_stride = rows over BIG_VOXELS[rows] voxels, with two chunks of 256 representatives in the first and the last of the
    rows that take one voxel each, a chunk of none in the middle of the rows behind them, and, where the last chunk holds one row,
    that row a representative.  -> (cloud, voxels, the empty chunk)"""
    voxels, chunks = BIG_VOXELS[rows], -(-rows // 256)
    c = vc.make_cloud(_rng(13, rows), rows, rows, SIZE, voxels, side=BIG_SIDE)
    lead = voxels // 256  # chunks whose rows take one voxel each
    empty = (lead + 1 + chunks) // 2
    vc.plant_chunk_counts(c, voxels, (1, lead - 1), (empty,))
    if rows % 256 == 1:
        c["n_opt"][rows - 1] = vc.HIGHEST_N_OPT
    return c, voxels, empty


_shared = {}


def _cloud_131073():
    """the two-wave cloud, shared by the tests that read it (none of them writes to it)"""
    if "c" not in _shared:
        _shared["c"] = _big_cloud(131073)
    return _shared["c"]


@pytest.mark.parametrize("rows", sorted(BIG_VOXELS))
def test_scan_beyond_one_wave_and_one_tile(hip_ctx, rows):
    """every output byte, both positions, run and count-only, at the four sizes either side of the scan's two switches.  What each
    case is there for is asserted on the restatement's result before anything is launched.  At the two sizes above 2 million rows
    the time goes to the host: about 1 s to seed the cloud and 1 to 1.6 s for each of the restatement's four results"""
    c, voxels, empty = _big_cloud(rows) if rows != 131073 else _cloud_131073()
    chunks, large = -(-rows // 256), rows > 1 << 20
    assert chunks == {131072: 512, 131073: 513, 2097152: 8192, 2097153: 8193}[rows]
    keep = (lambda names: tuple(k for k in names if k != "desc")) if large else tuple
    inputs, outputs = keep(INPUTS), keep(ops.WorldVoxelBatch.OPTIONAL)
    table_stride = 1 << voxels.bit_length()  # the next power of two above the voxel count: 2^17 and 2^21 slots
    out_stride = voxels + 3
    known = {}
    for position in POSITIONS:
        p = ops.world_voxel_params(SIZE, position)
        known[p.position, False] = expected_of([c], inputs, p, out_stride, table_stride)
        w = known[p.position, False][0]
        assert w["status"] == ref.PRS_OK and w["n_out"] == w["n_voxels"] == voxels and w["count"].sum() == rows
        counts, bases = vc.chunk_counts(w["index"], chunks)
        assert counts.min() == 0 and counts.max() == 256 and ((counts > 0) & (counts < 256)).any()
        assert 0 < empty < chunks - 1 and counts[empty] == 0 and counts[:empty].all() and counts[empty + 1:].all()
        assert bases[-1] > (1 << 20 if large else 1 << 16)
        if rows % 256 == 1:  # the last chunk holds one row and it represents its voxel
            assert counts[-1] == 1 and bases[-1] == voxels - 1 and w["index"][bases[-1]] == rows - 1
        if rows == 2097153:  # chunk 8192 is the first of the second tile: its base is the carry alone
            assert chunks - 1 == 8192 and w["index"][bases[8192]] >= 2097152
    rig = Rig(hip_ctx, [c], out_stride, table_stride, outputs, inputs, known)
    rig.check_both(SIZE, "rows %d" % rows)
    rig.check_both(SIZE, "rows %d, count only" % rows, count_only=True)


def test_truncation_at_a_large_base(hip_ctx):
    """out_stride one below the voxel count, with the cut in a chunk whose base is above 2^16"""
    c, voxels, _ = _cloud_131073()
    table_stride, inputs = 1 << voxels.bit_length(), INPUTS
    known = {}
    for position in POSITIONS:
        p = ops.world_voxel_params(SIZE, position)
        full = expected_of([c], inputs, p, voxels, table_stride)[0]
        known[p.position, False] = expected_of([c], inputs, p, voxels - 1, table_stride)
        w = known[p.position, False][0]
        assert (w["status"], w["n_out"], w["n_voxels"]) == (ref.PRS_ERR_CAPACITY, voxels - 1, voxels)
        assert w["index"].tolist() == full["index"][:-1].tolist() and w["index"][-1] > 1 << 16
        assert full["index"][-1] == 131072  # the row that is cut off: the one row of the last chunk
    rig = Rig(hip_ctx, [c], voxels - 1, table_stride, known=known)
    rig.check_both(SIZE)


def test_all_rows_of_two_waves_of_chunks_in_one_voxel(hip_ctx):
    """131073 rows on one slot: the rank's row index passes 2^16 and the MEAN divides sums of 131073 terms of up to 2^30"""
    c = vc.one_voxel_cloud(_rng(14), 131073, 131073, SIZE)
    c["n_opt"][70000], c["n_opt"][100000] = 9, 9  # the tie goes to the lower row
    known = {}
    for position in POSITIONS:
        p = ops.world_voxel_params(SIZE, position)
        known[p.position, False] = expected_of([c], INPUTS, p, 5, 1 << 18)
        w = known[p.position, False][0]
        assert w["n_voxels"] == 1 and w["index"].tolist() == [70000] and w["count"].tolist() == [131073]
    rig = Rig(hip_ctx, [c], 5, 1 << 18, known=known)
    rig.check_both(SIZE)


@pytest.mark.parametrize("position", POSITIONS)
def test_a_short_sequence_beside_a_long_one(hip_ctx, position):
    """B = 2 with 131073 and 2305 rows in one in_stride: the scan's workgroup is sized by the stride, the short sequence's result is
    what it is alone"""
    long_, voxels, _ = _cloud_131073()
    short = vc.make_cloud(_rng(15), 131073, 2305, SIZE, 500)
    p = ops.world_voxel_params(SIZE, position)
    rig2 = Rig(hip_ctx, [long_, short], voxels + 3, 1 << 18)
    want = rig2.check(p)
    assert [w["n_voxels"] for w in want] == [voxels, 500]
    both = _snapshot(rig2, 1)
    rig1 = Rig(hip_ctx, [short], voxels + 3, 1 << 18)
    rig1.check(p)
    assert _snapshot(rig1, 0) == both


def test_rank_key_at_the_extremes_of_n_opt(hip_ctx):
    """n_opt 0, 1, 2^31 - 1, 2^31 and 2^32 - 1 inside the same voxels: the complement and the shift that pack the rank"""
    values = [0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
    c = vc.make_cloud(_rng(16), 2305, 2305, SIZE, 300)
    vc.spread_n_opt(_rng(16, 1), c, SIZE, values)
    assert c["n_opt"].dtype == np.uint32 and sorted(set(c["n_opt"].tolist())) == values
    known = {}
    for position in POSITIONS:
        p = ops.world_voxel_params(SIZE, position)
        known[p.position, False] = expected_of([c], INPUTS, p, 2305, 8192)
        w = known[p.position, False][0]
        assert w["n_voxels"] == 300 and sorted(set(w["n_opt"].tolist())) == values  # every value wins somewhere
        # and loses somewhere: voxels whose best row is not their first hold every value but the lowest
        later = w["index"] >= 300
        assert sorted(set(w["n_opt"][later].tolist())) == values[1:]
    rig = Rig(hip_ctx, [c], 2305, 8192, known=known)
    rig.check_both(SIZE)


def test_call_level_refusals_write_nothing(hip_ctx):
    c = vc.make_cloud(_rng(11), 300, 257, SIZE, 60)
    rig = Rig(hip_ctx, [c, c], 300)
    lib, ctx = _lib.load(), hip_ctx._h
    D = lambda: rig.vx.descriptor(rig.cloud())  # noqa: E731

    def run(d, p=None):
        p = ops.world_voxel_params(SIZE, "mean") if p is None else p
        return lib.prs_world_voxel_batch_run(ctx, C.byref(p) if p != "null" else None, C.byref(d) if d is not None else None)

    assert run(D()) == 0
    hip_ctx.synchronize()
    rig.fill_sentinel()
    assert run(None) == -1 and run(D(), "null") == -1
    for field in ("in_xyz", "in_n", "n_out", "n_voxels", "n_nonfinite", "n_outside", "status", "workspace"):
        d = D()
        setattr(d, field, None)
        assert run(d) == -1, field
    for field, value in (("batch", 0), ("in_stride", 0), ("in_stride", -5), ("table_stride", 0), ("table_stride", 768), ("table_stride", -1024),
                         ("out_stride", 0), ("out_stride", -1)):
        d = D()
        setattr(d, field, value)
        assert run(d) == ref.PRS_ERR_RANGE, (field, value)
    for size, position in ((0.0, 0), (-1.0, 0), (float("nan"), 0), (float("inf"), 1), (0.3, 2), (0.3, -1)):
        p = _lib.WorldVoxelParams()
        p.voxel_size, p.position = size, position
        assert run(D(), p) == ref.PRS_ERR_RANGE, (size, position)
    for field, step in (("in_xyz", 8), ("in_desc", 8), ("xyz", 8), ("desc", 8), ("workspace", 8), ("in_n", 2), ("in_n_opt", 1), ("in_node", 2),
                        ("in_row", 2), ("index", 2), ("count", 1), ("node", 2), ("row", 2), ("n_opt", 2), ("n_out", 2), ("n_voxels", 1),
                        ("n_nonfinite", 2), ("n_outside", 2), ("status", 2)):
        d = D()
        setattr(d, field, getattr(d, field) + step)
        assert run(d) == -5, field
    hip_ctx.synchronize()
    for k, v in rig.outputs().items():
        assert (v.view(np.uint8) == SENTINEL).all(), k
    d = D()
    d.xyz, d.out_stride = None, 0  # legal in a count-only call
    assert run(d) == 0
    hip_ctx.synchronize()


@pytest.mark.parametrize("position", POSITIONS)
def test_captured_graph_replayed_after_the_inputs_change(hip_ctx, position):
    import torch
    ctx = hip_ctx
    clouds = [vc.make_cloud(_rng(12, b), 600, n, SIZE, 100) for b, n in enumerate((515, 0, 600))]
    rig = Rig(ctx, clouds, 300, table_stride=256)
    p = ops.world_voxel_params(SIZE, position)
    cloud = rig.cloud()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        rig.vx.run(ctx, p, cloud)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rig.vx.run(ctx, p, cloud)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    torch.cuda.synchronize()
    # other rows, other voxel counts, a sequence that overflows its table and one that is refused: the table left by one replay is
    # cleared by the next
    shapes = [((257, 90), (600, 300), (64, 7)), ((600, 256), (601, 5), (1, 1))]
    for replay, shape in enumerate(shapes):
        for b, (n, voxels) in enumerate(shape):
            rig.clouds[b] = vc.make_cloud(_rng(12, replay, b), 600, n, SIZE, voxels)
        rig.upload()
        rig.fill_sentinel()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = rig.expected(p)
        rig.compare(rig.outputs(), want, "replay %d" % replay)
        assert [w["n_voxels"] for w in want] == ([90, -1, 7] if replay == 0 else [256, 0, 1])


def test_from_maps_archived_by_the_session_itself(hip_ctx):
    """one chain end to end: ReentryBatch.step archives two finished maps per sequence, WorldMapBatch.run exports the cloud, and
    WorldVoxelBatch.run reads the world map's tensors in place.  Against the restatement applied to the world-map restatement's cloud"""
    import world_map_cases as wc
    import world_map_ref as wref
    from test_reentry_gpu import Rig as ReentryRig, _walk
    from test_world_map_gpu import _push
    rr_rig = ReentryRig(hip_ctx, 2, 6, 40, 4, 6, handover_stride=40, slot_stride=3, max_measurements=2)
    _walk(rr_rig, np.random.default_rng(11))
    rng = np.random.default_rng(12)
    X = rr_rig.graphs.X.cpu().numpy().reshape(2, -1, 4, 4).copy()
    for b in range(2):
        for n in range(3):
            X[b, n] = X[b, n] @ np.linalg.inv(np.asarray(wc.rigid(rng, scale=0.05)).reshape(4, 4))
    _push(rr_rig.graphs.X, X.reshape(rr_rig.graphs.X.shape))
    rr_rig.maps.n_points.fill_(7)
    wm = ops.WorldMapBatch(rr_rig.sess, rr_rig.maps, rr_rig.arch, 200)
    wp = dict()  # every row
    wm.run(hip_ctx, ops.world_map_params(**wp))
    vx = ops.WorldVoxelBatch(2, 200, 200)
    assert vx.table_stride == 512
    size = 1.5  # the walk's landmarks are a few metres apart
    for position, mode in zip(POSITIONS, (ref.REPRESENTATIVE, ref.MEAN)):
        vx.run(hip_ctx, ops.world_voxel_params(size, position), wm)
        hip_ctx.synchronize()
        for b in range(2):
            archived = [(n, rr_rig.arch.slot_of(b, n)) for n in range(2)]
            live = (2, dict(coords=rr_rig.maps.coords[b].cpu().numpy(), n_opt=rr_rig.maps.n_opt[b].cpu().numpy(),
                            inlier=rr_rig.maps.inlier[b].cpu().numpy(), n_points=int(rr_rig.maps.n_points[b].item())))
            xyz = wref.host_route(archived, live, X[b].reshape(-1, 16), wref.params(**wp))
            mapped = wm.cloud_of(b)  # n_opt, desc, node and row of the same rows: the world map's tests compare them
            assert mapped["xyz"].tobytes() == xyz.tobytes() and xyz.shape[0] > 7  # more than the live map's rows
            n = xyz.shape[0]
            pad = lambda a: np.concatenate([a, np.zeros((200 - n,) + a.shape[1:], a.dtype)])  # noqa: E731
            c = dict(in_stride=200, n=n, xyz=pad(xyz), **{k: pad(mapped[k]) for k in INPUTS})
            want = ref.world_voxel(c, ref.params(size, mode), 200, 512)
            got = vx.cloud_of(b)
            assert want["status"] == ref.PRS_OK and 1 < want["n_voxels"] < n  # some rows are fused, not all into one
            assert (got["status"], got["n_out"], got["n_voxels"], got["n_total"]) == (ref.PRS_OK,) + (want["n_voxels"],) * 3
            for k in ROW_OUTPUTS:
                assert got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (position, b, k)
    rr_rig.close()
