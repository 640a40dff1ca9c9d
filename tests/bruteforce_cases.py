"""Inputs of exactly known content for the brute-force matcher's tests.

Independent random 256-bit rows are 128 +- 8 bits apart (the closest of four million random pairs: 87 bits), so a cloud pair of random
rows holds no candidate at any threshold the pipeline uses.  The generators here put candidates where a test wants them:
shared_prototypes() draws both clouds from ONE prototype array (tie-heavy content: equal distances, shared best partners, pools with
conflicts); planted() derives chosen rows from a common base row with chosen bits flipped and CHECKS on the CPU that the pairs below
`floor` bits are exactly the planted ones, at exactly the planted distances (it redraws otherwise); conflict_chain() is a planted
pair of clouds whose result is written out by hand."""
import numpy as np

from bruteforce_ref import hamming_all


def random_rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip(row, bits):
    out = np.array(row, dtype=np.uint8, copy=True)
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def _noisy(rng, base, n, flips):
    """n rows, each a random prototype with 0..flips random bit flips (a bit drawn twice flips back)"""
    bits = np.unpackbits(base[rng.integers(0, base.shape[0], n)], axis=1)
    k = rng.integers(0, flips + 1, n)
    where = rng.integers(0, 256, (n, max(flips, 1)))
    for j in range(flips):
        rows = np.nonzero(k > j)[0]
        bits[rows, where[rows, j]] ^= 1
    return np.packbits(bits, axis=1)


def shared_prototypes(rng, n_base, nf, nm, flips):
    """-> (fixed [nf, 32], moving [nm, 32]): one prototype array, drawn once, for both clouds"""
    base = random_rows(rng, n_base)
    return _noisy(rng, base, nf, flips), _noisy(rng, base, nm, flips)


def planted(rng, nf, nm, plan, floor=80, tries=8):
    """-> (fixed, moving, expected {(f, m): d}).  Rows are random but for the planted ones.

    plan: a list of (f, m, d) -- moving row m is fixed row f with exactly d random bits flipped (entries sharing f share its row) --
    and / or groups dict(fixed={f: bits}, moving={m: bits}): every named row is one base row with the given bits flipped, so the
    distance of two rows of a group is the size of the symmetric difference of their bit sets.  `expected` holds every pair of a
    group closer than `floor`; the generator asserts that these are ALL the pairs below `floor`, at these distances."""
    for _ in range(tries):
        df, dm = random_rows(rng, nf), random_rows(rng, nm)
        groups, by_f = [], {}
        for item in plan:
            if isinstance(item, dict):
                groups.append(item)
                continue
            f, m, d = item
            if f not in by_f:
                by_f[f] = dict(fixed={f: ()}, moving={})
                groups.append(by_f[f])
            assert m not in by_f[f]["moving"]
            by_f[f]["moving"][m] = tuple(int(b) for b in rng.permutation(256)[:d])
        expected = {}
        seen_f, seen_m = set(), set()
        for g in groups:
            base = random_rows(rng, 1)[0]
            for f, bits in g["fixed"].items():
                assert 0 <= f < nf and f not in seen_f, f
                seen_f.add(f)
                df[f] = flip(base, bits)
            for m, bits in g["moving"].items():
                assert 0 <= m < nm and m not in seen_m, m
                seen_m.add(m)
                dm[m] = flip(base, bits)
            for f, bf in g["fixed"].items():
                for m, bm in g["moving"].items():
                    d = len(set(bf) ^ set(bm))
                    if d < floor:
                        expected[(f, m)] = d
        dist = hamming_all(df, dm)
        ff, mm = np.nonzero(dist < floor)
        found = {(int(f), int(m)): int(dist[f, m]) for f, m in zip(ff, mm)}
        if found == expected:
            return df, dm, expected
    raise AssertionError("no draw held exactly the planted pairs below %d bits" % floor)


def spread(rng, nf, nm, count, distances, floor=80, extra=()):
    """planted(): `count` <= nm candidates (f_i, m_i, d_i) with m_i = i, f_i = i % nf walking the fixed cloud and d_i cycling through
    `distances`; `extra`: further plan entries on other rows"""
    assert count <= nm
    return planted(rng, nf, nm, [(i % nf, i, distances[i % len(distances)]) for i in range(count)] + list(extra), floor)


# ---- the conflict chain -----------------------------------------------------------------------------------------------------
# One FIXED index (CHAIN_F) and one MOVING index (CHAIN_M) each take part in the pools of three consecutive non-empty levels
# (5, 18 and 20 bits), at ratio 0.9 and any threshold in (40, 80]:
#   level  5: two candidates share the index (a crossed tie): both are dropped for the conflict (:256-266);
#   level 18: one candidate, unique in its pool, but 18 / 20 == 0.9f is not < 0.9: Lowe rejects it on the chain's side (:281-286);
#   level 20: one candidate, 20 / 40 < 0.9, its partner's list holds it alone: registered (:287-290);
#   level 40: the chain's index is registered, the candidate never enters a pool (:112-113).
# On the device the pool counts of consecutive non-empty levels alternate between the 16-bit halves of a count word and are cleared
# lazily: the count of 2 left by level 5 must be gone when level 20 counts into the same half.
CHAIN_F, CHAIN_F_PARTNERS = 3, {1: 5, 4: 5, 6: 18, 7: 20, 9: 40}      # moving index -> distance to fixed CHAIN_F
CHAIN_M, CHAIN_M_PARTNERS = 11, {0: 5, 2: 5, 5: 18, 8: 20, 10: 40}    # fixed index -> distance to moving CHAIN_M
CHAIN_RATIO = 0.9
CHAIN_EXPECTED = [(3, 7, 20.0), (8, 11, 20.0)]  # (fixed, moving, response) in the canonical order
CHAIN_CANDIDATES, CHAIN_LEVELS, CHAIN_DROPPED, CHAIN_LOWE_FIXED, CHAIN_LOWE_MOVING = 10, 4, 4, 1, 1


def conflict_chain(rng, nf=12, nm=12, shift_f=0, shift_m=0):
    """-> (fixed, moving): the chain above in clouds of nf x nm otherwise random rows, its indices shifted by (shift_f, shift_m)"""
    def bits(d, first):
        return tuple(range(first, first + d))
    # disjoint bit ranges per partner: the partners' mutual distances do not matter (they lie in the same cloud)
    g_f = dict(fixed={CHAIN_F + shift_f: ()}, moving={})
    g_m = dict(moving={CHAIN_M + shift_m: ()}, fixed={})
    first = 0
    for m, d in CHAIN_F_PARTNERS.items():
        g_f["moving"][m + shift_m] = bits(d, first)
        first += d
    first = 0
    for f, d in CHAIN_M_PARTNERS.items():
        g_m["fixed"][f + shift_f] = bits(d, first)
        first += d
    df, dm, expected = planted(rng, nf, nm, [g_f, g_m])
    assert len(expected) == CHAIN_CANDIDATES
    return df, dm


def chain_expected(shift_f=0, shift_m=0):
    return [(f + shift_f, m + shift_m, r) for f, m, r in CHAIN_EXPECTED]
