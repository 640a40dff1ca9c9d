"""Every kernel the brute-force matcher's dispatch can launch, on inputs that hold candidates, against the C oracle AND the plain-Python
reference (tests/bruteforce_ref.py), through the device-resident batch entry of the C-ABI.

bruteforce_plan (csrc/bruteforce.hip) chooses among 15 kernels: bruteforce_kernel<KPT, MODE> for KPT 1 / 2 / 4 / 8 x
{fused, dense, register}, the two matrix-core fused shapes (1024 and 512 threads) and bruteforce_dense_mfma_kernel.  DISPATCH holds
one row per path: the kernels it was written for (as a kernel trace prints them), a builder of its cloud pairs -- a row may size its
batch by the device's CU count -- and what it claims to exercise.  Every row first asserts that tests/bruteforce_dispatch.py, the
restatement of the host's choice, and the library's own plan name the row's kernels for this device, then compares matches, their order, n_matches and status
of every pair bit for bit with the oracle, and of every pair (batches up to 16 pairs) or of the edge pairs and one pair in eight (larger
batches) with the Python reference.  tests/test_bruteforce_dispatch_table.py checks without a GPU that the variant table names no
kernel without a row, that the restatement equals the library's plan and that every row holds the content it claims: candidates, pool conflicts, Lowe rejections, at least three
distance levels, candidate counts on the stated side of `cap` / `lvl_cap`, second row passes, segment drains and flushes."""
import zlib

import numpy as np
import pytest

import bruteforce_cases as bc
import bruteforce_dispatch as bd
import bruteforce_ref as br
from helpers import corr_equal
from srrg2_proslam_amd import ops

pytestmark = pytest.mark.gpu

ERR_CAPACITY = -2
TWO = "PRS_BF_TWO_WORKGROUPS"
K = bd.kernel_name
FUSED_MX, FUSED_MX_512 = K(1, bd.FUSED, True), K(1, bd.FUSED, True, 512)


class Case:
    """the cloud pairs of one row: pairs = [(fixed rows, moving rows, content key)]; pairs of equal key hold equal content (their
    expectations are computed once); n_raw[b] = the (n_fixed, n_moving) the device is told when they differ from the rows given"""

    def __init__(self, fs, ms, mode, launches, pairs, cap=0, env=None, n_raw=None, edges=()):
        self.fs, self.ms, self.mode, self.launches, self.cap, self.env = fs, ms, mode, launches, cap, dict(env or {})
        self.pairs = [(p[0], p[1], p[2] if len(p) > 2 else ("pair", i)) for i, p in enumerate(pairs)]
        self.n_raw = dict(n_raw or {})
        self.edges = set(edges) | {0, len(pairs) - 1}
        self.name = None

    def dispatch(self, cus, max_dist):
        return bd.dispatch(len(self.pairs), self.fs, self.ms, max_dist, self.cap, self.mode, cus, self.env)

    def clamped(self, b):
        df, dm, _ = self.pairs[b]
        if b in self.n_raw:
            nf, nm = self.n_raw[b]
            df, dm = df[: min(max(nf, 0), self.fs)], dm[: min(max(nm, 0), self.ms)]
        return df, dm

    def referenced(self, b):
        return len(self.pairs) <= 16 or b in self.edges or b % 8 == 0


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def tie_pair(rng, nf, nm, n_base=100, flips=12, plant_last=True):
    """both clouds from one prototype array; the LAST rows of both clouds are a planted match 3 bits apart (a popcount thread's last
    owned row, the last row of the last tile / wave / pass / chunk / slice)"""
    df, dm = bc.shared_prototypes(rng, n_base, nf, nm, flips)
    if plant_last and nf and nm:
        r = bc.random_rows(rng, 1)[0]
        df[nf - 1] = r
        dm[nm - 1] = bc.flip(r, rng.permutation(256)[:3])
    return df, dm


def near_matrix(df, dm, max_dist):
    return br.hamming_all(df, dm) < bd.limit_of(max_dist)


def cells_per_wave(near, rows_wg, first_col=0, n_cols=None):
    """per wave of a workgroup owning fixed rows [0, rows_wg): the (4-row group, moving column) cells that hold a candidate in the
    columns [first_col, first_col + n_cols) -- a lower bound of the entries the matrix-core kernels park there (one per cell)"""
    nf, nm = near.shape
    last = nm if n_cols is None else min(nm, first_col + n_cols)
    out = []
    for r0 in range(0, min(nf, rows_wg), 64):
        blk = near[r0:min(r0 + 64, nf), first_col:last]
        pad = (-blk.shape[0]) % 4
        blk = np.concatenate([blk, np.zeros((pad, blk.shape[1]), bool)]) if pad else blk
        out.append(int(blk.reshape(-1, 4, blk.shape[1]).any(axis=1).sum()))
    return out


_EXPECT = {}


def expectation(oracle, case, b, max_dist, ratio, cap, want_ref):
    """-> dict(n_cand, ref (matches, flags), stats | None, oracle (matches, flags)) of one pair at one launch; cached by content"""
    df, dm = case.clamped(b)
    key = (case.name, case.pairs[b][2], df.shape[0], dm.shape[0], float(max_dist), float(ratio), cap)
    e = _EXPECT.get(key)
    if e is None:
        e = dict(n_cand=int(np.count_nonzero(near_matrix(df, dm, max_dist))) if len(df) and len(dm) else 0, stats=None, ref=None)
        e["overflow"] = e["n_cand"] > cap
        if e["overflow"]:
            e["oracle"] = (np.zeros(0, dtype=ops.CORR_DTYPE), ERR_CAPACITY)
        else:
            e["oracle"] = oracle.bruteforce_match(df, dm, max_dist, ratio)
        _EXPECT[key] = e
    if want_ref and e["ref"] is None:
        m, flags, stats = br.match(df, dm, max_dist, ratio)
        assert stats["candidates"] == e["n_cand"]
        e["stats"] = stats
        e["ref"] = (np.zeros(0, dtype=ops.CORR_DTYPE), ERR_CAPACITY) if e["overflow"] else (m, flags)
    return e


DISPATCH = []


def row(id, kernels, make, **claims):
    def named(cus):
        case = make(cus)
        case.name = id  # (content keys are the row's own)
        return case

    DISPATCH.append(dict(id=id, kernels=list(kernels), make=named, claims=claims))


# ---- 1. the twelve popcount instantiations ------------------------------------------------------------------------------------
# fixed stride -> the sizes of the fixed clouds (on and either side of a multiple of 1024 where the stride allows)
POPCOUNT_SHAPES = {1024: (1024, 1023, 1), 1025: (1025, 1024, 1023), 2048: (2048, 2047, 1025), 2049: (2049, 2048, 2047),
                   4096: (4096, 4095, 3073), 4097: (4097, 4096, 4095), 8192: (8192, 8191, 7169)}


def _kpt(fs):
    return 1 if fs <= 1024 else (2 if fs <= 2048 else (4 if fs <= 4096 else 8))


def _popcount_row(fs, split):
    name = "popcount_%s_%d" % ("split" if split else "fused", fs)
    ms, nms = (300, (300, 299, 33)) if split else (200, (200, 199, 97))

    def make(cus):
        rng = _rng(name)
        return Case(fs, ms, bd.POPCOUNT, [(20.0, 0.9)], [tie_pair(rng, nf, nm) for nf, nm in zip(POPCOUNT_SHAPES[fs], nms)])

    kernels = [K(_kpt(fs), bd.DENSE), K(_kpt(fs), bd.REGISTER)] if split else [K(_kpt(fs), bd.FUSED)]
    # (the fused popcount shape is taken at any batch size below a moving stride of 256; three pairs * 2 <= cus: the split shape)
    row(name, kernels, make, conflicts=True, lowe=True, levels3=True, last_row_match=True)


for _fs in POPCOUNT_SHAPES:
    _popcount_row(_fs, False)
    _popcount_row(_fs, True)


# ---- 2. the split shape's slices ------------------------------------------------------------------------------------------------
def _make_split_slices(cus):
    rng = _rng("split_slices")
    sizes = [(1024, 2600), (500, 10), (1, 1), (64, 31), (1000, 32), (77, 33), (1023, 2599)]
    return Case(1024, 2600, bd.POPCOUNT, [(20.0, 0.9)], [tie_pair(rng, nf, nm) for nf, nm in sizes])


row("split_slices", [K(1, bd.DENSE), K(1, bd.REGISTER)], _make_split_slices, conflicts=True, lowe=True, levels3=True, last_row_match=True,
    empty_slices=True, ragged_slices=True)


# ---- 3. the split matrix-core kernel ---------------------------------------------------------------------------------------------
def _make_mfma_edges(cus):
    rng = _rng("mfma_edges")
    sizes = [(15, 63), (16, 64), (17, 65), (63, 127), (64, 129), (65, 64), (1023, 63), (1024, 65), (1025, 129)]
    return Case(1025, 300, bd.MATRIX, [(20.0, 0.9)], [tie_pair(rng, nf, nm, n_base=30) for nf, nm in sizes])


def _make_mfma_flush(cus):
    rng = _rng("mfma_flush")
    return Case(1100, 300, bd.MATRIX, [(16.0, 0.9)], [tie_pair(rng, 1100, 300, n_base=8, flips=10), tie_pair(rng, 64, 129, n_base=8, flips=10)],
                cap=65536)


row("mfma_edges", [bd.MFMA_KERNEL, K(2, bd.REGISTER)], _make_mfma_edges, conflicts=True, lowe=True, levels3=True, last_row_match=True)
row("mfma_flush", [bd.MFMA_KERNEL, K(2, bd.REGISTER)], _make_mfma_flush, conflicts=True, lowe=True, levels3=True, last_row_match=True,
    mid_cloud_flush=0)


# ---- 4. the fused matrix-core shapes --------------------------------------------------------------------------------------------
NM_EDGES = (129, 64, 63, 65, 127, 128, 200, 31, 33, 32)


def _fused_matrix_row(name, kernel, fs, ms, nf_lo, batch_of, env, contents, threads, mode=bd.MATRIX_WHEN_FULL, cap=40000, n_base=8):
    def make(cus):
        rng = _rng(name)
        pool = []
        for i in range(contents):
            nf = fs if i == 0 else (nf_lo if i == 1 else int(rng.integers(nf_lo, fs + 1)))
            nm = min(NM_EDGES[i % len(NM_EDGES)], ms)
            pool.append(tie_pair(rng, nf, nm, n_base=n_base, flips=12) + (("content", i),))
        B = batch_of(cus)
        return Case(fs, ms, mode, [(20.0, 0.9), (50.0, 0.8)], [pool[b % contents] for b in range(B)], cap=cap, env=env,
                    edges=(1, B - 2, cus - 1, cus, 2 * cus - 1, 2 * cus))

    row(name, [kernel], make, conflicts=True, lowe=True, levels3=True, last_row_match=True, second_pass=threads, drains=threads)


_fused_matrix_row("fused_matrix_1024_switch_off", FUSED_MX, 1300, 200, 1025, lambda cus: 40, {TWO: "0"}, 10, 1024)
_fused_matrix_row("fused_matrix_512_switch_on", FUSED_MX_512, 600, 200, 513, lambda cus: 40, {TWO: "1"}, 10, 512)
_fused_matrix_row("fused_matrix_1024_by_batch", FUSED_MX, 1300, 200, 1025, lambda cus: min(max(32, cus // 4), cus), {}, 10, 1024)  # 32 or more
_fused_matrix_row("fused_matrix_512_by_batch", FUSED_MX_512, 600, 64, 513, lambda cus: cus + 8, {}, 10, 512, cap=16384)         # more than cus
_fused_matrix_row("fused_matrix_512_looping", FUSED_MX_512, 520, 64, 513, lambda cus: 2 * cus + 5, {}, 12, 512, cap=8192)       # more than 2 * cus
_fused_matrix_row("fused_matrix_1024_looping", FUSED_MX, 1030, 64, 1025, lambda cus: cus + 5, {TWO: "0"}, 8, 1024, cap=16384)
_fused_matrix_row("fused_matrix_forced_small", FUSED_MX, 1030, 200, 1025, lambda cus: 3, {}, 3, 1024, mode=bd.MATRIX)          # (moving stride < 256)


# ---- 5. the registration-state forks --------------------------------------------------------------------------------------------
def _make_global_split(cus):
    rng = _rng("global_split")
    return Case(2048, 2048, bd.POPCOUNT, [(256.0, 0.9)], [tie_pair(rng, 250, 240, n_base=40), tie_pair(rng, 100, 255, n_base=40)], cap=65536)


def _make_global_fused(cus):
    rng = _rng("global_fused")
    return Case(8192, 255, bd.POPCOUNT, [(256.0, 0.9)], [tie_pair(rng, 300, 200, n_base=40), tie_pair(rng, 150, 255, n_base=40)], cap=65536)


row("global_state_split", [K(2, bd.DENSE), K(2, bd.REGISTER)], _make_global_split, conflicts=True, lowe=True, levels3=True,
    facts=dict(bm_fits=False, lvl_cap=0))
row("global_state_fused", [K(8, bd.FUSED)], _make_global_fused, conflicts=True, lowe=True, levels3=True, facts=dict(bm_fits=False, lvl_cap=0))

LVL_FS, LVL_MS, LVL_THRESHOLD = 4096, 8192, 32.0  # one bitmap word: the bitmaps take 48 KiB, 8184 candidates keep their lists in LDS
_LVL = {}


def _lvl_pairs():
    """a pair with exactly lvl_cap candidates, one with lvl_cap + 1, and a small one"""
    if not _LVL:
        lvl_cap = bd.dispatch(2, LVL_FS, LVL_MS, LVL_THRESHOLD, 0, bd.POPCOUNT, 256)["lvl_cap"]
        assert lvl_cap == 8184
        rng = _rng("lvl_edge")
        # every fixed row meets 8 moving rows, all at different distances 0..31 (31 = lim - 1)
        for name, count in (("at", lvl_cap), ("above", lvl_cap + 1)):
            df, dm, expected = bc.spread(rng, 1023, LVL_MS, count, list(range(32)), floor=72)
            assert len(expected) == count
            _LVL[name] = (df, dm, ("lvl", name))
        _LVL["small"] = bc.conflict_chain(rng, 40, 50) + (("lvl", "small"),)
    return _LVL


def _make_lvl_split(cus):
    p = _lvl_pairs()
    return Case(LVL_FS, LVL_MS, bd.POPCOUNT, [(LVL_THRESHOLD, 0.9)], [p["at"], p["above"]])


def _make_lvl_fused(cus):
    p = _lvl_pairs()
    B = cus + 2  # workgroup 0: lvl_cap + 1 (lists in global memory), then lvl_cap (LDS); workgroup 1 the other way round
    pairs = [p["small"]] * B
    pairs[0], pairs[1], pairs[cus], pairs[cus + 1] = p["above"], p["at"], p["at"], p["above"]
    return Case(LVL_FS, LVL_MS, bd.POPCOUNT, [(LVL_THRESHOLD, 0.9)], pairs, edges=(1, cus, cus + 1))


row("level_lists_split", [K(4, bd.DENSE), K(4, bd.REGISTER)], _make_lvl_split, levels3=True, lvl_edge=(0, 1),
    facts=dict(bm_fits=True, lvl_cap=8184, nw=1))
row("level_lists_fused", [K(4, bd.FUSED)], _make_lvl_fused, lowe=True, levels3=True, lvl_edge=(1, 0), facts=dict(bm_fits=True, lvl_cap=8184, nw=1))


# ---- 6. capacity -----------------------------------------------------------------------------------------------------------------
CAP = 64


def _cap_contents(rng, nf, nm):
    out = {}
    for name, count in (("exact", CAP), ("over", CAP + 1), ("some", 40)):
        df, dm, expected = bc.spread(rng, nf, nm, count, [0, 3, 7, 12, 19])
        assert len(expected) == count
        out[name] = (df, dm, ("cap", name))
    out["chain"] = bc.conflict_chain(rng, min(nf, 40), min(nm, 40)) + (("cap", "chain"),)
    return out


def _capacity_row(name, kernels, fs, ms, mode, env, looping):
    def make(cus):
        c = _cap_contents(_rng(name), min(fs, 300), min(ms, 100))
        if looping:
            # workgroup w takes the pairs w, w + grid, ..: an overflowing pair is followed by a good one and the other way round
            # (more pairs than workgroups: cus, or 2 * cus in the 512-thread shape)
            B = cus + 3
            if bd.dispatch(B, fs, ms, 50.0, CAP, mode, cus, env)["grid"] == B:
                B = 2 * cus + 3
            grid = bd.dispatch(B, fs, ms, 50.0, CAP, mode, cus, env)["grid"]
            assert B == grid + 3
            pairs = [c["some"] if b % 2 else c["chain"] for b in range(B)]
            pairs[0], pairs[1], pairs[2] = c["over"], c["exact"], c["chain"]
            pairs[grid], pairs[grid + 1], pairs[grid + 2] = c["some"], c["over"], c["exact"]
            return Case(fs, ms, mode, [(50.0, 0.9)], pairs, cap=CAP, env=env, edges=(1, 2, grid, grid + 1, grid + 2))
        return Case(fs, ms, mode, [(50.0, 0.9)], [c["over"], c["exact"], c["chain"], c["some"]], cap=CAP, env=env)

    row(name, kernels, make, at_cap=True, above_cap=True, after_overflow=looping)


_capacity_row("capacity_fused_popcount", [K(1, bd.FUSED)], 300, 100, bd.POPCOUNT, {}, True)
_capacity_row("capacity_split_popcount", [K(1, bd.DENSE), K(1, bd.REGISTER)], 300, 300, bd.POPCOUNT, {}, False)
_capacity_row("capacity_split_matrix", [bd.MFMA_KERNEL, K(1, bd.REGISTER)], 300, 300, bd.MATRIX, {}, False)
_capacity_row("capacity_fused_matrix_1024", [FUSED_MX], 300, 100, bd.MATRIX_WHEN_FULL, {TWO: "0"}, True)
_capacity_row("capacity_fused_matrix_512", [FUSED_MX_512], 300, 100, bd.MATRIX_WHEN_FULL, {TWO: "1"}, True)


def _make_capacity_default(cus):
    """candidate_capacity = 0 means 16 * max(stride) = 528 = 16 x 33 candidates; 23 x 23 = 529 are one too many"""
    rng = _rng("capacity_default")
    same = lambda idx: {i: () for i in idx}
    at = bc.planted(rng, 33, 33, [dict(fixed=same(range(16)), moving=same(range(33)))])
    above = bc.planted(rng, 33, 33, [dict(fixed=same(range(10, 33)), moving=same(range(23)))])
    assert len(at[2]) == 528 and len(above[2]) == 529
    return Case(33, 33, bd.POPCOUNT, [(50.0, 0.9)], [at[:2], above[:2], bc.conflict_chain(rng, 33, 33)])


row("capacity_default_rule", [K(1, bd.FUSED)], _make_capacity_default, at_cap=True, above_cap=True, facts=dict(cap=528))


# ---- 7. thresholds and ratios ----------------------------------------------------------------------------------------------------
# (best, second) pairs whose float32 quotient EQUALS the ratio: the strict `<` rejects them; 31 / 32 and 63 / 64: the second best lies
# in the next bitmap word
RATIO_EDGES = {0.9: [(9, 10), (18, 20), (27, 30), (36, 40), (45, 50)], 0.5: [(1, 2)], 0.8: [(4, 5)], 0.95: [(19, 20)]}
WORD_EDGES = [(31, 32), (63, 64)]
THRESHOLDS = (0.0, -1.0, 1.0, 32.0, 33.0, 64.0, 65.0, 255.5, 256.0)
RATIOS = (0.9, 0.0, 0.5, 0.8, 0.95, 1.0, 1.5)


def boundary_pair(rng, nf=150, nm=150):
    """-> (fixed, moving, index): every (best, second) pair above once on the fixed side (fixed row f meets two moving rows at the two
    distances) and once on the moving side; index[(best, second)] = ((f, m_best, m_second), (m, f_best, f_second))"""
    plan, index = [], {}
    f = m = 0
    for best, second in [p for ps in RATIO_EDGES.values() for p in ps] + WORD_EDGES:
        plan.append(dict(fixed={f: ()}, moving={m: tuple(range(best)), m + 1: tuple(range(100, 100 + second))}))
        plan.append(dict(moving={m + 2: ()}, fixed={f + 1: tuple(range(best)), f + 2: tuple(range(100, 100 + second))}))
        index[(best, second)] = ((f, m, m + 1), (m + 2, f + 1, f + 2))
        f, m = f + 3, m + 3
    df, dm, _ = bc.planted(rng, nf, nm, plan)
    return df, dm, index


def _make_thresholds(mode):
    def make(cus):
        rng = _rng("thresholds")
        b = boundary_pair(rng)
        pairs = [(b[0], b[1]), bc.conflict_chain(rng, 12, 12), tie_pair(rng, 150, 140, n_base=10, flips=40)]
        launches = [(70.0, r) for r in RATIOS] + [(t, 0.9) for t in THRESHOLDS]
        return Case(160, 160, mode, launches, pairs, cap=32768)
    return make


row("thresholds_and_ratios_popcount", [K(1, bd.FUSED)], _make_thresholds(bd.POPCOUNT), conflicts=True, lowe=True, levels3=True)
row("thresholds_and_ratios_matrix", [FUSED_MX], _make_thresholds(bd.MATRIX), conflicts=True, lowe=True, levels3=True)


def far_moving_pair(rng, nf, nm):
    """planted matches all along a long moving cloud: every fixed row but the last six meets four moving rows at four different
    distances below 32 (9 / 10 among them: a Lowe rejection on the fixed side), a crossed tie on either side, a Lowe rejection on the
    moving side, and a match in the last moving row"""
    ds = [0, 2, 5, 9, 10, 20, 27, 31]
    g = nf - 6
    taken, plan = {nm - 1, nm - 2, nm - 3, 8191, 8192}, []
    for i in range(4 * g):
        f, m = i % g, (i * 997 + 13) % nm
        while m in taken:
            m = (m + 1) % nm
        taken.add(m)
        plan.append((f, m, ds[(i // g + f) % 8]))
    plan.append(dict(moving={nm - 3: ()}, fixed={g: tuple(range(9)), g + 1: tuple(range(20, 30))}))          # 9 / 10 on the moving side
    plan += [(g + 2, 8191, 4), (g + 2, 8192, 4)]                                                             # a crossed tie on the fixed side
    plan.append(dict(moving={nm - 2: ()}, fixed={g + 3: tuple(range(6)), g + 4: tuple(range(10, 16))}))      # ... and on the moving side
    plan.append((g + 5, nm - 1, 1))
    return bc.planted(rng, nf, nm, plan)[:2]


def _make_far_moving(ms, fused):
    def make(cus):
        rng = _rng("far_moving_%d" % ms)
        far = far_moving_pair(rng, 64, ms) + (("far", ms),)
        if not fused:
            return Case(64, ms, bd.POPCOUNT, [(32.0, 0.9)], [far])
        B = cus // 2 + 1
        small = bc.conflict_chain(rng, 30, 40) + (("far", "small"),)
        return Case(64, ms, bd.POPCOUNT, [(32.0, 0.9)], [far if b % 3 == 0 else small for b in range(B)], cap=4096)
    return make


row("far_moving_lds_lists", [K(1, bd.DENSE), K(1, bd.REGISTER)], _make_far_moving(16000, False), conflicts=True, lowe=True, levels3=True,
    far_match=True, facts=dict(bm_fits=True))
row("far_moving_global_lists", [K(1, bd.DENSE), K(1, bd.REGISTER)], _make_far_moving(20000, False), conflicts=True, lowe=True, levels3=True,
    far_match=True, facts=dict(bm_fits=False))
row("far_moving_fused", [K(1, bd.FUSED)], _make_far_moving(16000, True), conflicts=True, lowe=True, levels3=True, far_match=True,
    facts=dict(bm_fits=True))


# ---- 8. cloud sizes out of range ---------------------------------------------------------------------------------------------------
def _clamp_row(name, kernels, fs, ms, mode):
    def make(cus):
        rng = _rng(name)
        pairs = [tie_pair(rng, fs, ms, n_base=20, plant_last=False) for _ in range(5)]
        n_raw = {0: (-1, 50), 1: (fs + 7, ms + 100), 2: (40, -5), 3: (2 ** 30, 30), 4: (fs, ms)}
        return Case(fs, ms, mode, [(20.0, 0.9)], pairs, n_raw=n_raw)

    row(name, kernels, make, conflicts=True, lowe=True, levels3=True)


_clamp_row("sizes_clamped_popcount", [K(1, bd.FUSED)], 100, 90, bd.POPCOUNT)
_clamp_row("sizes_clamped_split_matrix", [bd.MFMA_KERNEL, K(1, bd.REGISTER)], 100, 300, bd.MATRIX)
_clamp_row("sizes_clamped_fused_matrix", [FUSED_MX], 100, 90, bd.MATRIX)


# ---- what a row claims, from the reference (no GPU: tests/test_bruteforce_dispatch_table.py runs this for 256 CUs) -----------------
def check_claims(r, case, cus, oracle):
    claims = r["claims"]
    max_dist, ratio = case.launches[0]
    d = case.dispatch(cus, max_dist)
    assert d["refused"] is None and d["kernels"] == r["kernels"], (r["id"], d)
    assert d["scratch_bytes"] < 2 ** 31, r["id"]
    for k, v in claims.get("facts", {}).items():
        assert d[k] == v, (r["id"], k, d[k])
    keys, total = set(), dict(candidates=0, dropped=0, lowe_fixed=0, lowe_moving=0, matches=0, levels=0)
    for b in range(len(case.pairs)):
        e = expectation(oracle, case, b, max_dist, ratio, d["cap"], case.referenced(b))
        if e["stats"] is None or case.pairs[b][2] in keys:
            continue
        keys.add(case.pairs[b][2])
        df, dm = case.clamped(b)
        if len(df) > 1 and len(dm) > 1:
            assert e["n_cand"] > 0, (r["id"], b)
        if not e["overflow"]:
            for k in ("candidates", "dropped", "lowe_fixed", "lowe_moving", "matches"):
                total[k] += e["stats"][k]
            total["levels"] = max(total["levels"], e["stats"]["levels"])
            assert corr_equal(e["ref"][0], e["oracle"][0]) and e["ref"][1] == e["oracle"][1], (r["id"], b)
        if claims.get("last_row_match") and len(df) and len(dm):
            m = e["ref"][0]
            assert ((m["fixed_idx"] == len(df) - 1) & (m["moving_idx"] == len(dm) - 1) & (m["response"] == 3.0)).any(), (r["id"], b)
    assert total["candidates"] > 0 and total["matches"] > 0, r["id"]
    if claims.get("conflicts"):
        assert total["dropped"] > 0, r["id"]
    if claims.get("lowe"):
        assert total["lowe_fixed"] > 0 and total["lowe_moving"] > 0, r["id"]
    if claims.get("levels3"):
        assert total["levels"] >= 3, r["id"]
    n_cand = [expectation(oracle, case, b, max_dist, ratio, d["cap"], False)["n_cand"] for b in range(len(case.pairs))]
    if claims.get("at_cap"):
        assert d["cap"] in n_cand, r["id"]
    if claims.get("above_cap"):
        assert d["cap"] + 1 in n_cand, r["id"]
    if claims.get("after_overflow"):
        # a workgroup's next pair behind an overflowing one holds candidates and must come out right
        over = [b for b, n in enumerate(n_cand) if n > d["cap"]]
        assert any(b + d["grid"] < len(n_cand) and 0 < n_cand[b + d["grid"]] <= d["cap"] for b in over), r["id"]
    if "lvl_edge" in claims:
        at, above = claims["lvl_edge"]
        assert n_cand[at] == d["lvl_cap"] and n_cand[above] == d["lvl_cap"] + 1 and d["lvl_cap"] < d["cap"], r["id"]
    if claims.get("empty_slices") or claims.get("ragged_slices"):
        assert d["chunks"] > 1
        slices = [bd.split_slices(len(case.clamped(b)[1]), d["chunks"]) for b in range(len(case.pairs))]
        assert any(s0 >= s1 for sl in slices for s0, s1 in sl), r["id"]
        assert any(s1 > s0 and (s1 - s0) % 32 for sl in slices for s0, s1 in sl), r["id"]
        for nm in (1, 31, 32, 33):
            assert any(len(case.clamped(b)[1]) == nm for b in range(len(case.pairs))), r["id"]
    if "mid_cloud_flush" in claims:
        df, dm = case.clamped(claims["mid_cloud_flush"])
        assert d["mfma"] and len(dm) > bd.MFMA_CHUNK
        near = near_matrix(df, dm, max_dist)
        # a wave's segment holds at least kBfmFlushAt entries behind the first 64-row chunk, with chunks to follow
        assert max(cells_per_wave(near, bd.MFMA_ROWS_WG, 0, bd.MFMA_CHUNK)) >= bd.MFMA_FLUSH_AT, r["id"]
    if "second_pass" in claims:
        threads, found_pass, found_drains = claims["second_pass"], False, False
        assert d["fused_matrix"] and d["dual"] == (threads == 512), r["id"]
        for b in sorted({b for b in range(len(case.pairs)) if case.referenced(b)})[:16]:
            df, dm = case.clamped(b)
            near = near_matrix(df, dm, max_dist)
            found_pass |= bool(near[threads:].any())
            # a drain empties at most kMxSeg entries: more than two segments' worth in one wave's pass = drained more than once
            found_drains |= max(cells_per_wave(near, threads)) > 2 * bd.MX_SEG
        assert found_pass and found_drains, r["id"]
    if claims.get("far_match"):
        m = expectation(oracle, case, 0, max_dist, ratio, d["cap"], True)["ref"][0]
        nm = len(case.clamped(0)[1])
        assert (m["moving_idx"] > 8191).any() and (m["moving_idx"] == nm - 1).any(), r["id"]
        assert n_cand[0] <= d["lvl_cap"] or not d["bm_fits"], r["id"]
    return d


# ---- the device ---------------------------------------------------------------------------------------------------------------------
def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _context(case, monkeypatch):
    for name in ("PRS_BF_GLOBAL_STATE", TWO):
        if name in case.env:
            monkeypatch.setenv(name, case.env[name])
        else:
            monkeypatch.delenv(name, raising=False)
    ctx = ops.Context(0)
    ctx.set_bruteforce_dense_phase(case.mode)
    return ctx


def _upload(case):
    clouds = ops.BruteforceClouds(0, len(case.pairs), case.fs, case.ms, candidate_capacity=case.cap)
    sent = {}
    for b, (df, dm, key) in enumerate(case.pairs):
        if key in sent:  # equal content: a copy on the device
            clouds.fixed_desc[b].copy_(clouds.fixed_desc[sent[key]])
            clouds.moving_desc[b].copy_(clouds.moving_desc[sent[key]])
            clouds.n_fixed[b], clouds.n_moving[b] = len(df), len(dm)
        else:
            clouds.upload(b, df, dm)
            sent[key] = b
        if b in case.n_raw:
            clouds.n_fixed[b], clouds.n_moving[b] = case.n_raw[b]
    return clouds


@pytest.mark.parametrize("r", DISPATCH, ids=[r["id"] for r in DISPATCH])
def test_dispatch_row(oracle, monkeypatch, r):
    import torch
    cus = _cus()
    case = r["make"](cus)
    check_claims(r, case, cus, oracle)
    ctx = _context(case, monkeypatch)
    try:
        clouds = _upload(case)
        for max_dist, ratio in case.launches:
            d = case.dispatch(cus, max_dist)
            assert d["refused"] is None and d["kernels"] == r["kernels"], (max_dist, d)
            # ... and so does the library's own plan for these inputs on this context (host only)
            assert ops.bruteforce_plan(ops.bruteforce_params(max_dist, ratio), clouds.descriptor(), ops.dispatch_env(ctx))["kernels"] == r["kernels"]
            clouds.n_matches.fill_(-7)
            clouds.status.fill_(-7)
            ops.bruteforce_match_batch(ctx, ops.bruteforce_params(max_dist, ratio), clouds)
            ctx.synchronize()
            torch.cuda.synchronize()
            n_matches, status = clouds.n_matches.cpu().numpy(), clouds.status.cpu().numpy()
            raw = clouds.matches.cpu().numpy()
            for b in range(len(case.pairs)):
                e = expectation(oracle, case, b, max_dist, ratio, d["cap"], case.referenced(b))
                got = np.zeros(max(int(n_matches[b]), 0), dtype=ops.CORR_DTYPE)
                got["fixed_idx"], got["moving_idx"] = raw[b, : len(got), 0], raw[b, : len(got), 1]
                got["response"] = raw[b, : len(got), 2].view(np.float32)
                for name in ("oracle", "ref"):
                    if e[name] is not None:
                        want, flags = e[name]
                        where = (r["id"], b, max_dist, ratio, name)
                        assert int(n_matches[b]) == len(want), where
                        assert corr_equal(want, got), where
                        assert int(status[b]) == flags, where
    finally:
        ctx.close()


REFUSALS = [
    ("stride", dict(fs=8193, ms=16)),
    ("stride", dict(fs=16, ms=65536)),
    ("threshold", dict(fs=64, ms=64, max_dist=256.5)),
    ("lds", dict(fs=8192, ms=30000)),
]


@pytest.mark.parametrize("why,shape", REFUSALS, ids=["fixed_stride_8193", "moving_stride_65536", "threshold_256_5", "lds"])
def test_refusals_launch_nothing(why, shape):
    import torch
    fs, ms, max_dist = shape["fs"], shape["ms"], shape.get("max_dist", 50.0)
    assert bd.dispatch(1, fs, ms, max_dist, 0, bd.MATRIX_WHEN_FULL, _cus())["refused"] == why
    ctx = ops.Context(0)
    try:
        clouds = ops.BruteforceClouds(0, 1, fs, ms)
        df, dm = bc.conflict_chain(_rng("refusals"), 12, 12)
        clouds.upload(0, df, dm)
        clouds.n_matches.fill_(-7)
        clouds.status.fill_(-7)
        with pytest.raises(ops.ProslamHipError) as err:
            ops.bruteforce_match_batch(ctx, ops.bruteforce_params(max_dist, 0.9), clouds)
        assert err.value.status == bd.ERR_UNSUPPORTED and bd.REFUSALS[why] in str(err.value)
        ctx.synchronize()
        torch.cuda.synchronize()
        assert int(clouds.n_matches[0].item()) == -7 and int(clouds.status[0].item()) == -7  # nothing ran
    finally:
        ctx.close()


def test_conflict_chain_by_hand(oracle):
    """the hand-written expectation of bruteforce_cases.conflict_chain, on the fused popcount, fused matrix and split shapes, the
    chain at the first and at the last indices of its clouds"""
    import torch
    for mode, ms in ((bd.POPCOUNT, 200), (bd.MATRIX, 200), (bd.POPCOUNT, 300), (bd.MATRIX, 300)):
        ctx = ops.Context(0)
        ctx.set_bruteforce_dense_phase(mode)
        try:
            rng = _rng("chain")
            clouds = ops.BruteforceClouds(0, 2, 1100, ms)
            shifts = [(0, 0), (1100 - 12, ms - 12)]
            for b, (sf, sm) in enumerate(shifts):
                clouds.upload(b, *bc.conflict_chain(rng, 12 + sf, 12 + sm, sf, sm))
            ops.bruteforce_match_batch(ctx, ops.bruteforce_params(50.0, bc.CHAIN_RATIO), clouds)
            ctx.synchronize()
            torch.cuda.synchronize()
            for b, (sf, sm) in enumerate(shifts):
                got = clouds.matches_of(b)
                assert [(int(c["fixed_idx"]), int(c["moving_idx"]), float(c["response"])) for c in got] == bc.chain_expected(sf, sm), (mode, ms, b)
                assert int(clouds.status[b].item()) == 0
        finally:
            ctx.close()
