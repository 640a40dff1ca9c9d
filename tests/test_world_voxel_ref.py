"""The numpy restatement of the world voxel filter (tests/world_voxel_ref.py) means what the header says: known answers, worked out by
hand, for floor against truncation, the edge of the grid, the representative, both positions, the order and the counts.  No GPU
needed."""
import numpy as np
import pytest

import world_voxel_cases as vc
import world_voxel_ref as ref

F = np.float32


def _cloud(xyz3, n_opt=None, n=None):
    xyz3 = np.asarray(xyz3, F).reshape(-1, 3)
    N = xyz3.shape[0]
    xyz = np.concatenate([xyz3, np.arange(N, dtype=F)[:, None] + F(0.5)], axis=1)
    return dict(in_stride=N, n=N if n is None else n, xyz=xyz, n_opt=None if n_opt is None else np.asarray(n_opt, np.uint32))


def test_floor_not_truncation():
    s = np.float64(vc.EDGE_SIZE)
    for value, fate in vc.EDGES:
        if isinstance(fate, int):
            assert ref.voxel_index(value, s) == fate, (value, fate)
    # truncation would put the first three into voxel 0 with +1e-30; floor separates them
    out = ref.world_voxel(_cloud([[-1e-30, 0, 0], [1e-30, 0, 0], [-0.0, 0, 0], [-0.5, 0, 0], [-0.5000001, 0, 0]]), ref.params(0.5), 8)
    assert out["n_voxels"] == 3 and out["index"].tolist() == [0, 1, 4] and out["count"].tolist() == [2, 2, 1]


def test_the_edge_of_the_grid():
    s, last, first_out = F(0.5), F(524287.75), F(524288.0)
    below = np.nextafter(F(-524288.0), F(-np.inf))
    out = ref.world_voxel(_cloud([[last, 0, 0], [first_out, 0, 0], [0, -524288.0, 0], [0, below, 0], [0, 0, 3e38], [np.nan, 0, 0],
                                  [0, np.inf, first_out]]), ref.params(s), 8)
    assert (out["n_voxels"], out["n_outside"], out["n_nonfinite"]) == (2, 3, 2)  # a row that is both counts as not finite
    assert out["index"].tolist() == [0, 2]
    keys = ref.voxel_key(np.array([[(1 << 20) - 1] * 3, [-(1 << 20)] * 3]))
    assert int(keys[0]) == (1 << 63) - 1 and int(keys[1]) == 0  # below 2^63: all ones never is a key


def test_the_representative():
    # three rows of one voxel, two of another
    xyz = [[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3], [1.1, 0, 0], [1.2, 0, 0]]
    rep = lambda n_opt: ref.world_voxel(_cloud(xyz, n_opt), ref.params(1.0), 8)["index"].tolist()  # noqa: E731
    assert rep([0, 5, 3, 1, 1]) == [1, 3]  # the greatest n_opt; among equals the smallest row
    assert rep([4, 4, 4, 0, 7]) == [0, 4]
    assert rep([0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]) == [2, 3]
    assert rep(None) == [0, 3]  # no n_opt: every row has 0
    assert int(ref.rank_key(0xFFFFFFFF, 7)) == 7 and int(ref.rank_key(0, 7)) == (0xFFFFFFFF << 32) | 7
    out = ref.world_voxel(_cloud(xyz, [0, 5, 3, 1, 1]), ref.params(1.0), 8)
    assert out["count"].tolist() == [3, 2] and out["n_opt"].tolist() == [5, 1]
    assert out["xyz"].tobytes() == _cloud(xyz)["xyz"][[1, 3]].tobytes()  # four floats, bit for bit


def _ulp(x):
    x = np.abs(np.asarray(x, F))
    return np.maximum(np.nextafter(x, F(np.inf)) - x, np.nextafter(F(0), F(1)))


@pytest.mark.parametrize("s", [0.3, 0.5, 1e-3, 40.0])
def test_mean_of_one_row_is_that_row(s):
    rng = np.random.default_rng(7)
    c = vc.make_cloud(rng, 500, 500, s, 500)
    out = ref.world_voxel(c, ref.params(s, ref.MEAN), 500)
    assert out["n_voxels"] == 500 and out["index"].tolist() == list(range(500))
    # q_a rounds the fraction to 2^-30 of a voxel (below a float ulp of the coordinate here), the final (float) rounds once
    assert (np.abs(out["xyz"][:, :3].astype(np.float64) - c["xyz"][:, :3]) <= _ulp(c["xyz"][:, :3])).all()
    assert out["xyz"][:, 3].tobytes() == c["xyz"][:, 3].tobytes()


def test_mean_stays_inside_its_voxel():
    rng = np.random.default_rng(8)
    s = F(0.3)
    c = vc.make_cloud(rng, 3000, 3000, s, 40)
    # rows hard against both faces of their voxel
    k = ref.voxel_index(c["xyz"][:, :3], np.float64(s))
    c["xyz"][:1000, :3] = (k[:1000] * np.float64(s)).astype(F)
    c["xyz"][1000:2000, :3] = np.nextafter(((k[1000:2000] + 1) * np.float64(s)).astype(F), F(-np.inf))
    out = ref.world_voxel(c, ref.params(s, ref.MEAN), 3000)
    k_rep = ref.voxel_index(c["xyz"][out["index"], :3], np.float64(s))
    lo, hi = k_rep * np.float64(s), (k_rep + 1) * np.float64(s)
    m = out["xyz"][:, :3].astype(np.float64)
    assert (m >= lo - _ulp(lo)).all() and (m <= hi + _ulp(hi)).all()
    # and it is the mean: against a plain float64 average of the voxel's rows, to the quantisation (2^-30 of a voxel per row) and a rounding
    keys = ref.voxel_key(ref.voxel_index(c["xyz"][:, :3], np.float64(s)).astype(np.int64))
    for j in (0, 7, out["n_voxels"] - 1):
        rows = keys == keys[out["index"][j]]
        plain = c["xyz"][rows, :3].astype(np.float64).mean(axis=0)
        assert out["count"][j] == rows.sum() and (np.abs(m[j] - plain) <= 2 * _ulp(plain) + float(s) * 2.0 ** -29).all()


def test_mean_does_not_depend_on_the_order_of_the_rows():
    rng = np.random.default_rng(9)
    c = vc.one_voxel_cloud(rng, 2305, 2305, 0.3)
    c["n_opt"][...] = 0
    a = ref.world_voxel(c, ref.params(0.3, ref.MEAN), 4)
    d = dict(c, xyz=c["xyz"][::-1].copy())
    b = ref.world_voxel(d, ref.params(0.3, ref.MEAN), 4)
    assert a["count"].tolist() == b["count"].tolist() == [2305]
    assert a["xyz"][0, :3].tobytes() == b["xyz"][0, :3].tobytes()


def test_output_is_a_subsequence_and_counts_add_up():
    rng = np.random.default_rng(10)
    c = vc.make_cloud(rng, 2400, 2305, vc.EDGE_SIZE, 300)
    planted = vc.plant_edges(c, range(5, 2305, 61))
    for position in (ref.REPRESENTATIVE, ref.MEAN):
        out = ref.world_voxel(c, ref.params(vc.EDGE_SIZE, position), 2400)
        assert out["status"] == ref.PRS_OK and (np.diff(out["index"]) > 0).all() and out["index"].max() < 2305
        assert out["count"].sum() == 2305 - out["n_nonfinite"] - out["n_outside"]
        assert out["n_nonfinite"] == sum(f == "nonfinite" for _, _, f in planted)
        assert out["n_outside"] == sum(f == "outside" for _, _, f in planted)
        for k in ("desc", "node", "row", "n_opt"):
            assert out[k].tobytes() == c[k][out["index"]].tobytes()
        # node-then-row order is kept
        order = out["node"].astype(np.int64) * 1000 + out["row"]
        assert (np.diff(order) > 0).all()
    rep = ref.world_voxel(c, ref.params(vc.EDGE_SIZE), 2400)
    assert rep["xyz"].tobytes() == c["xyz"][rep["index"]].tobytes()


def test_truncation_count_only_table_and_refusal():
    rng = np.random.default_rng(11)
    c = vc.make_cloud(rng, 300, 257, 0.3, 64)
    p = ref.params(0.3)
    full = ref.world_voxel(c, p, 300, table_stride=64)
    assert full["status"] == ref.PRS_OK and full["n_voxels"] == full["n_out"] == 64
    cut = ref.world_voxel(c, p, 63, table_stride=64)
    assert (cut["status"], cut["n_out"], cut["n_voxels"]) == (ref.PRS_ERR_CAPACITY, 63, 64)
    assert cut["index"].tolist() == full["index"][:63].tolist()
    counted = ref.world_voxel(c, p, None, table_stride=64)
    assert (counted["status"], counted["n_out"], counted["n_voxels"], counted["xyz"].shape) == (ref.PRS_OK, 0, 64, (0, 4))
    over = ref.world_voxel(c, p, 300, table_stride=32)
    assert (over["status"], over["n_out"], over["n_voxels"]) == (ref.PRS_ERR_CAPACITY, 0, -1)
    for n in (-1, 301):
        bad = ref.world_voxel(dict(c, n=n), p, 300)
        assert (bad["status"], bad["n_out"], bad["n_voxels"], bad["n_nonfinite"], bad["n_outside"]) == (ref.PRS_ERR_RANGE, 0, 0, 0, 0)
    empty = ref.world_voxel(dict(c, n=0), p, 300)
    assert (empty["status"], empty["n_out"], empty["n_voxels"]) == (ref.PRS_OK, 0, 0)
