"""Seeded inputs shared by the world map's tests (tests/world_map_ref.py is the restatement they are compared with)."""
import numpy as np

F = np.float32


def rigid(rng, scale=100.0):
    """a float64 node pose [16]: a random rotation (QR of a normal matrix, det forced to +1) and a translation of about `scale` m"""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3] = q
    T[:3, 3] = rng.normal(size=3) * scale
    return T.reshape(16)


def make_sequence(rng, capacity, slot_stride, node_stride, n_nodes, cur_node, slot_of_node, slot_n_points, live_n_points,
                  identity_graph=False):
    """one sequence in the layout world_map_ref.world_map takes; every row of every array is filled (rows from n_points on too, so
    that a kernel reading past n_points shows)"""
    S, cap, NS = slot_stride, capacity, node_stride
    X = np.stack([np.eye(4).reshape(16) if identity_graph else rigid(rng) for _ in range(NS)])

    def rows(lead):
        return dict(coords=rng.normal(size=lead + (cap, 4)).astype(F) * F(20), desc=rng.integers(0, 256, lead + (cap, 32), dtype=np.uint8),
                    n_opt=rng.integers(0, 6, lead + (cap,)).astype(np.uint32), inlier=rng.integers(0, 2, lead + (cap,)).astype(np.uint8),
                    state=rng.normal(size=lead + (cap, 4)).astype(F))

    live, slots = rows(()), rows((S,))
    live["n_points"] = int(live_n_points)
    slots["n_points"] = np.asarray(slot_n_points, np.int32).reshape(S).copy()
    son = np.full(NS, -1, np.int32)
    son[:len(slot_of_node)] = slot_of_node
    return dict(capacity=cap, slot_stride=S, node_stride=NS, n_nodes=int(n_nodes), cur_node=int(cur_node), graph_X=X, slot_of_node=son,
                live=live, slots=slots)


def standard_sequence(rng, capacity, slot_stride, node_stride=8, with_slot_for_cur=True):
    """n_points 0, 1 and capacity among the maps, slots given to nodes in non-monotonic order, the current node in the middle"""
    S = slot_stride
    if S == 1:  # the current node first; its own slot, or the slot with the node behind it
        son = [0, -1, -1] if with_slot_for_cur else [-1, 0, -1]
        return make_sequence(rng, capacity, 1, node_stride, 3, 0, son, [capacity], capacity)
    # S = 5: nodes 0..5, slots in the order 3, 0, (4 or none: the current node), 1, none, 2
    son = [3, 0, 4 if with_slot_for_cur else -1, 1, -1, 2]
    # by slot: node 1 full, node 3 one row, node 5 (the last map) half full, node 0 (the first map) empty, the current node's old copy
    n_points = [capacity, 1, max(capacity // 2, 1), 0, max(capacity - 1, 0)]
    return make_sequence(rng, capacity, 5, node_stride, 6, 2, son, n_points, capacity)
