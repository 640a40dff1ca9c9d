"""Plain-Python restatement of CorrespondenceFinderDescriptorBasedBruteforce::compute
(CF/correspondence_finder_descriptor_based_bruteforce_impl.cpp:8-155, Lowe checks :157-199, pool processing :247-293), independent of
the C oracle and of the kernels: the SEQUENTIAL form of the source -- sorted candidates, the sliding pool with its two
registered-checks, the early exit, the trailing pool -- with none of the device's distance bitmaps, levels or counting sort.

match() returns the correspondences in the project's canonical order ((response, fixed, moving): the tie-break this build defines
for the source's unstable sort by response), the warning bits, and counters the tests use to prove that an input holds what it
claims to exercise."""
import bisect

import numpy as np

CORR_DTYPE = np.dtype([("fixed_idx", "<i4"), ("moving_idx", "<i4"), ("response", "<f4")])
WARN_EMPTY_INPUT, WARN_NO_MATCHES = 1, 2

POPCOUNT8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def hamming_all(desc_fixed, desc_moving, block=128):
    """[nf, nm] Hamming distances of 256-bit rows, by the byte table"""
    df = np.ascontiguousarray(desc_fixed, dtype=np.uint8).reshape(-1, 32)
    dm = np.ascontiguousarray(desc_moving, dtype=np.uint8).reshape(-1, 32)
    out = np.zeros((df.shape[0], dm.shape[0]), dtype=np.int32)
    for f0 in range(0, df.shape[0], block):
        x = df[f0:f0 + block, None, :] ^ dm[None, :, :]
        out[f0:f0 + block] = POPCOUNT8[x].sum(axis=2, dtype=np.int32)
    return out


def candidates(desc_fixed, desc_moving, max_dist):
    """(fixed, moving, distance) of every pair with float32(d) < float32(max_dist) (:53), in the canonical order"""
    d = hamming_all(desc_fixed, desc_moving)
    with np.errstate(invalid="ignore"):
        keep = d.astype(np.float32) < np.float32(max_dist)
    f, m = np.nonzero(keep)
    dd = d[f, m]
    order = np.lexsort((m, f, dd))
    return f[order].astype(np.int64), m[order].astype(np.int64), dd[order].astype(np.int64)


def _lowe(best, distances, ratio):
    """checkLowesRatio on the sorted distance list of one index (:180-199, :159-176)"""
    if len(distances) == 1:
        return True
    i = bisect.bisect_right(distances, best)  # the first strictly larger distance
    if i == len(distances):
        return False  # second best == best
    return bool(np.float32(best) / np.float32(distances[i]) < np.float32(ratio))


def match(desc_fixed, desc_moving, max_dist, ratio, early_exit=True):
    """-> (correspondences [CORR_DTYPE], warning bits, counters)

    counters: candidates, levels (distinct candidate distances), dropped (pool members sharing an index with another member),
    lowe_fixed / lowe_moving (unique pool members the ratio rejects on that side; both sides are evaluated), matches,
    early_exit (the loop left through :138-141 with candidates unvisited)."""
    df = np.ascontiguousarray(desc_fixed, dtype=np.uint8).reshape(-1, 32)
    dm = np.ascontiguousarray(desc_moving, dtype=np.uint8).reshape(-1, 32)
    nf, nm = df.shape[0], dm.shape[0]
    flags = WARN_EMPTY_INPUT if nf == 0 or nm == 0 else 0
    stats = dict(candidates=0, levels=0, dropped=0, lowe_fixed=0, lowe_moving=0, matches=0, early_exit=False)
    out = []
    cf, cm, cd = candidates(df, dm, max_dist) if nf and nm else ((), (), ())
    n = len(cf)
    stats["candidates"] = n
    stats["levels"] = len(set(np.asarray(cd).tolist()))
    if n == 1:  # :81-86
        out.append((int(cf[0]), int(cm[0]), int(cd[0])))
    elif n > 1:
        cf, cm, cd = cf.tolist(), cm.tolist(), cd.tolist()
        dist_f, dist_m = {}, {}
        for f, m, d in zip(cf, cm, cd):  # (visited in ascending distance: the lists come out sorted)
            dist_f.setdefault(f, []).append(d)
            dist_m.setdefault(m, []).append(d)
        reg_f, reg_m = set(), set()

        def process(pool):  # :247-293
            per_f, per_m = {}, {}
            for f, m, _ in pool:
                per_f[f] = per_f.get(f, 0) + 1
                per_m[m] = per_m.get(m, 0) + 1
            for f, m, d in pool:
                if per_f[f] != 1 or per_m[m] != 1:
                    stats["dropped"] += 1
                    continue
                ok_f, ok_m = _lowe(d, dist_f[f], ratio), _lowe(d, dist_m[m], ratio)
                stats["lowe_fixed"] += not ok_f
                stats["lowe_moving"] += not ok_m
                if ok_f and ok_m:
                    out.append((f, m, d))
                    reg_f.add(f)
                    reg_m.add(m)

        pool = [(cf[0], cm[0], cd[0])]
        for i in range(1, n):
            f, m, d = cf[i], cm[i], cd[i]
            if f not in reg_f and m not in reg_m:
                if pool and d == pool[-1][2]:
                    pool.append((f, m, d))
                else:
                    process(pool)
                    pool = []
                    if f not in reg_f and m not in reg_m:
                        pool.append((f, m, d))
            if early_exit and (len(reg_f) == nf or len(reg_m) == nm):
                stats["early_exit"] = i + 1 < n
                break
        if pool:
            process(pool)
    res = np.zeros(len(out), dtype=CORR_DTYPE)
    if out:
        o = np.asarray(out, dtype=np.int64)
        res["fixed_idx"], res["moving_idx"], res["response"] = o[:, 0], o[:, 1], o[:, 2].astype(np.float32)
    stats["matches"] = len(out)
    if not out:
        flags |= WARN_NO_MATCHES
    return res, flags, stats
