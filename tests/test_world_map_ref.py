"""The world map's numpy restatement (tests/world_map_ref.py) on hand-made answers, and formats.write_ply.  No GPU needed."""
import numpy as np
import pytest

import world_map_cases as wc
import world_map_ref as ref

F = np.float32


def _seq(capacity=6, slot_stride=3, node_stride=5, n_nodes=4, cur_node=3, son=(0, 1, -1, -1), slot_np=(3, 2, 0), live_np=2, seed=1,
         identity=True):
    s = wc.make_sequence(np.random.default_rng(seed), capacity, slot_stride, node_stride, n_nodes, cur_node, son, slot_np, live_np,
                         identity_graph=identity)
    for part in (s["live"], s["slots"]):
        part["n_opt"][...] = 3
        part["inlier"][...] = 1
    return s


def test_identity_graph_copies_the_coordinates():
    s = _seq()
    out = ref.world_map(s, ref.params(), 100)
    want = np.concatenate([s["slots"]["coords"][0, :3], s["slots"]["coords"][1, :2], s["live"]["coords"][:2]])
    assert out["status"] == ref.PRS_OK and out["n_out"] == out["n_total"] == 7 and out["n_nonfinite"] == 0
    assert out["xyz"].tobytes() == want.tobytes()
    assert out["node"].tolist() == [0, 0, 0, 1, 1, 3, 3] and out["row"].tolist() == [0, 1, 2, 0, 1, 0, 1]
    assert out["desc"].tobytes() == np.concatenate([s["slots"]["desc"][0, :3], s["slots"]["desc"][1, :2], s["live"]["desc"][:2]]).tobytes()
    assert out["n_opt"].dtype == np.uint32 and out["n_opt"].tolist() == [3] * 7


def test_kilometre_translation_keeps_the_millimetres():
    """X = a translation of 1000.001 m (not a float): the float64 route gives the correctly rounded sum, the float32 pose does not"""
    s = _seq(son=(0, -1, -1, -1), slot_np=(4, 0, 0), n_nodes=1, cur_node=0)
    X = np.eye(4)
    X[:3, 3] = [1000.001, -1000.001, 1000.003]
    s["graph_X"][0] = X.reshape(16)
    # row 1 is a landmark near the world's origin seen from a map a kilometre away (a loop closure): the sum cancels, and what the
    # float32 pose lost of the translation (2.3e-5 m at 1000 m) is most of what is left
    c = np.array([[0.0004, 0.0004, 0.0004, 1], [-1000.0, 1000.0, -1000.0, 7], [0.25, 0.125, 0.0625, -2], [-0.0007, 0.0009, 0.0002, 0]], F)
    s["slots"]["coords"][0, :4] = c
    out = ref.world_map(s, ref.params(include_live=False), 10)
    exact = (c[:, :3].astype(np.float64) + X[:3, 3]).astype(F)  # one rounding of the float64 sum (exact on row 1: Sterbenz)
    assert out["xyz"][:, :3].tobytes() == exact.tobytes() and out["xyz"][:, 3].tobytes() == c[:, 3].tobytes()
    assert out["xyz"][1, :3].tolist() == [F(1000.001 - 1000.0), F(1000.0 - 1000.001), F(1000.003 - 1000.0)]
    X32 = X.astype(F)
    single = np.stack([((X32[i, 0] * c[:, 0] + X32[i, 1] * c[:, 1]) + X32[i, 2] * c[:, 2]) + X32[i, 3] for i in range(3)], axis=1)
    assert single.dtype == F
    ulp = np.spacing(np.abs(exact))
    assert (np.abs(single.astype(np.float64) - exact.astype(np.float64))[1] > 1000 * ulp[1]).all()


def test_operation_order_is_the_written_one():
    s = _seq(identity=False, son=(0, -1, -1, -1), slot_np=(6, 0, 0), n_nodes=1, cur_node=0)
    X = s["graph_X"][0]
    out = ref.world_map(s, ref.params(include_live=False), 10)
    for r in range(6):
        x, y, z = (float(v) for v in s["slots"]["coords"][0, r, :3])
        for i in range(3):
            w = ((X[4 * i] * x + X[4 * i + 1] * y) + X[4 * i + 2] * z) + X[4 * i + 3]
            assert out["xyz"][r, i] == F(w)


def test_live_map_replaces_its_archived_slot():
    s = _seq(son=(0, 1, -1, 2), slot_np=(3, 2, 5), live_np=2)
    with_live = ref.world_map(s, ref.params(include_live=True), 100)
    assert with_live["node"].tolist() == [0, 0, 0, 1, 1, 3, 3]
    assert with_live["xyz"][5:].tobytes() == s["live"]["coords"][:2].tobytes()
    archived = ref.world_map(s, ref.params(include_live=False), 100)
    assert archived["node"].tolist() == [0, 0, 0, 1, 1] + [3] * 5
    assert archived["xyz"][5:].tobytes() == s["slots"]["coords"][2, :5].tobytes()
    # without a slot and without the live map the current node contributes nothing
    s["slot_of_node"][3] = -1
    assert ref.world_map(s, ref.params(include_live=False), 100)["node"].tolist() == [0, 0, 0, 1, 1]


def test_order_is_by_node_not_by_slot():
    s = _seq(son=(2, 0, 1, -1), slot_np=(1, 2, 3), live_np=0)
    out = ref.world_map(s, ref.params(), 100)
    assert out["node"].tolist() == [0, 0, 0, 1, 2, 2] and out["row"].tolist() == [0, 1, 2, 0, 0, 1]
    assert out["xyz"][:3].tobytes() == s["slots"]["coords"][2, :3].tobytes()


def test_every_filter():
    s = _seq(son=(0, -1, -1, -1), slot_np=(6, 0, 0), live_np=0)
    s["slots"]["n_opt"][0] = [0, 1, 2, 3, 4, 5]
    s["slots"]["inlier"][0] = [1, 0, 1, 0, 1, 0]
    assert ref.world_map(s, ref.params(min_n_opt=3), 10)["row"].tolist() == [3, 4, 5]
    assert ref.world_map(s, ref.params(require_inlier=True), 10)["row"].tolist() == [0, 2, 4]
    assert ref.world_map(s, ref.params(min_n_opt=3, require_inlier=True), 10)["row"].tolist() == [4]
    assert ref.world_map(s, ref.params(min_n_opt=6), 10)["n_total"] == 0
    s["slots"]["n_opt"][0, 5] = 0xFFFFFFFF  # unsigned comparison
    assert ref.world_map(s, ref.params(min_n_opt=0x80000000), 10)["row"].tolist() == [5]
    s["slots"]["n_points"][0] = 2  # rows from n_points on do not exist
    assert ref.world_map(s, ref.params(), 10)["row"].tolist() == [0, 1]
    # not finite: dropped and counted, but only when the row passes the other tests
    s["slots"]["n_points"][0] = 6
    s["slots"]["coords"][0, 1, 0] = np.inf
    s["slots"]["coords"][0, 4, 2] = np.nan
    out = ref.world_map(s, ref.params(), 10)
    assert out["row"].tolist() == [0, 2, 3, 5] and out["n_nonfinite"] == 2
    assert ref.world_map(s, ref.params(require_inlier=True), 10)["n_nonfinite"] == 1
    # a float64 sum that overflows float is not finite either
    s["graph_X"][0][3] = 3e38
    s["slots"]["coords"][0, 0, 0] = 3e38
    assert ref.world_map(s, ref.params(), 10)["n_nonfinite"] == 3


def test_truncation_and_count_only():
    s = _seq()
    full = ref.world_map(s, ref.params(), 7)
    assert full["status"] == ref.PRS_OK and full["n_out"] == 7
    cut = ref.world_map(s, ref.params(), 6)
    assert cut["status"] == ref.PRS_ERR_CAPACITY and cut["n_out"] == 6 and cut["n_total"] == 7
    assert cut["xyz"].tobytes() == full["xyz"][:6].tobytes() and cut["node"].tolist() == full["node"][:6].tolist()
    one = ref.world_map(s, ref.params(), 1)
    assert one["n_out"] == 1 and one["bounds"].tolist() == full["xyz"][0, :3].tolist() * 2
    count = ref.world_map(s, ref.params(), None)
    assert count["status"] == ref.PRS_OK and count["n_out"] == 0 and count["n_total"] == 7 and count["bounds"] is None
    assert count["xyz"].shape == (0, 4)


def test_bounds_with_a_planted_negative_zero():
    s = _seq(son=(0, -1, -1, -1), slot_np=(3, 0, 0), live_np=0)
    # a world coordinate is -0 only when every term of its sum is: x = -0, 0 * y and 0 * z with y, z < 0, and a translation of -0
    s["graph_X"][0][3] = -0.0
    s["slots"]["coords"][0, :3, :3] = [[-0.0, -1, -2], [0.0, -1, -2], [-0.0, -3, -1]]
    out = ref.world_map(s, ref.params(), 10)
    assert np.signbit(out["xyz"][:, 0]).tolist() == [True, False, True]  # the cloud keeps the sign
    assert out["bounds"].tobytes() == np.array([0, -3, -2, 0, -1, -1], F).tobytes()  # the bounds do not: +0 as min and as max
    nothing = ref.world_map(s, ref.params(min_n_opt=9), 10)
    assert nothing["bounds"].tolist() == [np.inf] * 3 + [-np.inf] * 3


def test_refresh_state():
    s = _seq(identity=False, son=(0, 1, -1, 2), slot_np=(3, 2, 5), live_np=2)
    s["slots"]["n_opt"][0, 1] = 0           # filtered out, refreshed all the same
    s["slots"]["coords"][0, 2, 1] = np.nan  # not finite: left alone
    before_live, before_slots = s["live"]["state"].copy(), s["slots"]["state"].copy()
    out = ref.world_map(s, ref.params(min_n_opt=1, refresh_state=True), 2)  # truncation does not limit the refresh
    assert s["live"]["state"].tobytes() == before_live.tobytes() and s["slots"]["state"].tobytes() == before_slots.tobytes()
    want_slots, want_live = before_slots.copy(), before_live.copy()
    for slot, node, n in ((0, 0, 3), (1, 1, 2)):
        want_slots[slot, :n, :3] = ref.world_rows(s["graph_X"][node], s["slots"]["coords"][slot, :n])
    want_slots[0, 2] = before_slots[0, 2]
    want_live[:2, :3] = ref.world_rows(s["graph_X"][3], s["live"]["coords"][:2])
    assert out["slot_state"].tobytes() == want_slots.tobytes() and out["live_state"].tobytes() == want_live.tobytes()
    assert out["slot_state"][2].tobytes() == before_slots[2].tobytes()  # the current node's old copy is not a chosen map
    same = ref.world_map(s, ref.params(refresh_state=True), None)       # legal in a count-only call
    assert same["slot_state"][0, :2].tobytes() == want_slots[0, :2].tobytes()
    off = ref.world_map(s, ref.params(), 10)
    assert off["slot_state"].tobytes() == before_slots.tobytes() and off["live_state"].tobytes() == before_live.tobytes()


@pytest.mark.parametrize("change", [dict(n_nodes=0), dict(n_nodes=6), dict(cur_node=-1), dict(cur_node=4), dict(live=7), dict(live=-1),
                                    dict(son=(0, 3)), dict(slot_np=(1, 7)), dict(slot_np=(1, -1)), dict(son=(1, 0))])
def test_range_errors(change):
    s = _seq(son=(0, 1, -1, -1))
    for k in ("n_nodes", "cur_node"):
        if k in change:
            s[k] = change[k]
    if "live" in change:
        s["live"]["n_points"] = change["live"]
    if "son" in change:
        s["slot_of_node"][change["son"][0]] = change["son"][1]
    if "slot_np" in change:
        s["slots"]["n_points"][change["slot_np"][0]] = change["slot_np"][1]
    out = ref.world_map(s, ref.params(refresh_state=True), 10)
    assert out["status"] == ref.PRS_ERR_RANGE and out["n_out"] == out["n_total"] == out["n_nonfinite"] == 0 and out["bounds"] is None
    assert out["slot_state"].tobytes() == s["slots"]["state"].tobytes() and out["live_state"].tobytes() == s["live"]["state"].tobytes()


def test_unused_entries_are_not_checked():
    s = _seq(son=(0, 1, -1, -1))
    s["slot_of_node"][4] = 99             # a node at or beyond n_nodes
    s["slots"]["n_points"][2] = -5        # a slot no node names
    s["slot_of_node"][3] = 77             # the current node's entry, replaced by the live map
    assert ref.world_map(s, ref.params(), 10)["status"] == ref.PRS_OK
    s["live"]["n_points"] = 99            # the live map is not read without include_live; the entry then counts
    assert ref.world_map(s, ref.params(include_live=False), 10)["status"] == ref.PRS_ERR_RANGE
    s["slot_of_node"][3] = -1
    assert ref.world_map(s, ref.params(include_live=False), 10)["status"] == ref.PRS_OK


def _read_ply(path):
    """a vertex-only binary little-endian PLY of float and uchar properties -> (xyz [n, 3], desc [n, 32] or None)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + 11
    head = raw[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    n = int(head[2].split()[2])
    props = [ln.split()[1:] for ln in head if ln.startswith("property ")]
    dt = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[kind]) for kind, name in props])
    rec = np.frombuffer(raw, dt, count=n, offset=end)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(F).reshape(n, 3)
    return xyz, (np.stack([rec["d%d" % i] for i in range(32)], axis=1) if len(props) > 3 else None)


def test_ply_round_trip(tmp_path):
    from srrg2_proslam_amd import formats
    s = _seq(identity=False)
    out = ref.world_map(s, ref.params(), 100)
    path = str(tmp_path / "cloud.ply")
    formats.write_ply(path, out["xyz"], out["desc"])
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n")].decode("ascii").split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 7"]
    assert head[3:6] == ["property float x", "property float y", "property float z"] and head[6] == "property uchar d0" and len(head) == 39
    assert len(raw) == raw.index(b"end_header\n") + 11 + 7 * (12 + 32)
    xyz, desc = _read_ply(path)
    assert xyz.tobytes() == np.ascontiguousarray(out["xyz"][:, :3]).tobytes() and desc.tobytes() == out["desc"].tobytes()
    formats.write_ply(path, out["xyz"][:, :3])
    xyz, desc = _read_ply(path)
    assert desc is None and xyz.tobytes() == np.ascontiguousarray(out["xyz"][:, :3]).tobytes()
    formats.write_ply(path, np.zeros((0, 4), F))
    assert _read_ply(path)[0].shape == (0, 3)
    with pytest.raises(ValueError):
        formats.write_ply(path, out["xyz"], out["desc"][:3])
