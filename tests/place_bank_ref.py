"""CPU restatement of the place bank (include/proslam_hip.h, prs_place_bank_*): B independent place_ref.Database objects, the
append statuses of the device kernel and the storage layout an arena holds after an append (what prs_place_db_add builds).
"""
import numpy as np

import place_ref as pr

OK, WARN_EMPTY_INPUT, ERR_CAPACITY, ERR_RANGE = 0, pr.WARN_EMPTY_INPUT, pr.ERR_CAPACITY, pr.ERR_RANGE


def padded(n):
    return (n + 15) // 16 * 16


def i32(v):
    """(int32_t) of a 64-bit difference"""
    return (int(v) + 2**31) % 2**32 - 2**31


class Bank:
    """batch databases of map_stride maps and row_stride rows (rounded up to 16) each"""

    def __init__(self, batch, map_stride, row_stride):
        self.batch, self.map_stride, self.row_stride = batch, map_stride, padded(row_stride)
        self.clear()

    def clear(self):
        self.dbs = [pr.Database() for _ in range(self.batch)]
        self.rows = [0] * self.batch          # stored rows with pads
        self.nodes = [[] for _ in range(self.batch)]

    def append_one(self, b, n_query, graph_id, desc, valid=None, xyz=None, query_stride=None, base=0):
        """the status of sequence b's append; on anything but OK nothing changes.  desc: at least n_query rows (the slot)"""
        db = self.dbs[b]
        if n_query == 0:
            return WARN_EMPTY_INPUT
        if n_query < 0 or graph_id < 0:
            return ERR_RANGE
        if query_stride is not None and n_query > query_stride:
            return ERR_CAPACITY
        if any(m["graph_id"] == graph_id for m in db.maps):
            return ERR_RANGE
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)[:n_query]
        v = None if valid is None else np.asarray(valid)[:n_query]
        nk = n_query if v is None else int(np.count_nonzero(v))
        if len(db.maps) == self.map_stride or self.rows[b] + padded(nk) > self.row_stride:
            return ERR_CAPACITY
        db.add(graph_id, desc, v, None if xyz is None else np.asarray(xyz, np.float32).reshape(-1, 3)[:n_query])
        self.rows[b] += padded(nk)
        self.nodes[b].append(i32(graph_id - base))
        return OK

    def append(self, items, query_stride=None, bases=None):
        """items[b]: dict(n_query, graph_id, desc, valid, xyz) -> the statuses"""
        return [self.append_one(b, it["n_query"], it["graph_id"], it["desc"], it.get("valid"), it.get("xyz"), query_stride,
                                0 if bases is None else bases[b]) for b, it in enumerate(items)]

    def sizes(self):
        maps = [len(d.maps) for d in self.dbs]
        big = [max([len(m["desc"]) for m in d.maps], default=0) for d in self.dbs]
        return np.array(maps, np.int32), np.array(self.rows, np.int32), np.array(big, np.int32)

    def query(self, b, P, graph_id, desc, valid=None, n_query=None, query_stride=None):
        """query b against database b alone (place_ref.Database.query and the slot-size statuses of the batch entry)"""
        db = self.dbs[b]
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc) if n_query is None else n_query
        bad = dict(status=0, index_query=db.index_query(graph_id), counts=np.zeros(len(db.maps), np.int64), candidates=[], corr=[])
        if graph_id < 0 or n < 0:
            bad["status"] = ERR_RANGE
            return bad
        if query_stride is not None and n > query_stride:
            bad["status"] = ERR_CAPACITY
            return bad
        return db.query(P, graph_id, desc[:n], None if valid is None else np.asarray(valid)[:n])

    def layout(self, b):
        """the arena of sequence b up to its live sizes: dict(desc [rows, 32], xyz [rows, 4], row_pidx [rows], tile_map [rows / 16],
        map_off, map_rows, map_gid, node_of_map)"""
        db, rows = self.dbs[b], self.rows[b]
        out = dict(desc=np.zeros((rows, 32), np.uint8), xyz=np.zeros((rows, 4), np.float32), row_pidx=np.full(rows, -1, np.int32),
                   tile_map=np.zeros(rows // 16, np.int32), map_off=[], map_rows=[], map_gid=[], node_of_map=list(self.nodes[b]))
        r = 0
        for i, m in enumerate(db.maps):
            n = len(m["desc"])
            out["desc"][r: r + n], out["xyz"][r: r + n, :3], out["row_pidx"][r: r + n] = m["desc"], m["xyz"], m["pidx"]
            out["tile_map"][r // 16: (r + padded(n)) // 16] = i
            out["map_off"].append(r)
            out["map_rows"].append(n)
            out["map_gid"].append(m["graph_id"])
            r += padded(n)
        return out

    def links(self, b, result, graph_id, max_candidates, base=0):
        """(candidates_flat [max_candidates], query_node) the query of sequence b writes"""
        flat = [b * self.map_stride + m for m in result["candidates"]] + [-1] * (max_candidates - len(result["candidates"]))
        node = i32(graph_id - base) if result["status"] >= 0 and result["candidates"] else -1
        return flat, node
