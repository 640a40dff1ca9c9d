"""tests/bruteforce_ref.py, the sequential Python restatement of the brute-force matcher, against the C oracle on every family of
inputs the GPU rows use, against expectations written out by hand, through its early exit, and on the float32 and threshold edges."""
import numpy as np
import pytest

import bruteforce_cases as bc
import bruteforce_ref as br
from helpers import corr_equal
from test_bruteforce_dispatch_gpu import RATIO_EDGES, THRESHOLDS, WORD_EDGES, boundary_pair, far_moving_pair, tie_pair


def both(oracle, df, dm, max_dist, ratio):
    m, flags, stats = br.match(df, dm, max_dist, ratio)
    om, oflags = oracle.bruteforce_match(df, dm, max_dist, ratio)
    assert corr_equal(m, om) and flags == oflags, (max_dist, ratio, len(m), len(om), flags, oflags)
    # the canonical order: (response, fixed, moving) ascending
    key = list(zip(m["response"].tolist(), m["fixed_idx"].tolist(), m["moving_idx"].tolist()))
    assert key == sorted(key)
    assert len(set(m["fixed_idx"].tolist())) == len(m) == len(set(m["moving_idx"].tolist()))  # a bijection
    return m, flags, stats


def triples(m):
    return [(int(c["fixed_idx"]), int(c["moving_idx"]), float(c["response"])) for c in m]


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("n_base,flips,max_dist,ratio", [(40, 6, 20.0, 0.9), (60, 40, 50.0, 0.9), (30, 30, 45.0, 0.85), (8, 12, 31.0, 0.8),
                                                           (100, 12, 12.0, 1.0)])
def test_shared_prototypes_against_the_oracle(oracle, seed, n_base, flips, max_dist, ratio):
    rng = np.random.default_rng(1000 + seed)
    nf, nm = int(rng.integers(1, 700)), int(rng.integers(1, 700))
    df, dm = bc.shared_prototypes(rng, n_base, nf, nm, flips)
    _, _, stats = both(oracle, df, dm, max_dist, ratio)
    assert stats["candidates"] > 0


def test_all_candidates_at_threshold_256(oracle):
    rng = np.random.default_rng(7)
    df, dm = bc.shared_prototypes(rng, 40, 300, 280, 6)
    _, _, stats = both(oracle, df, dm, 256.0, 1.5)
    assert stats["candidates"] == 300 * 280 and stats["levels"] > 30 and stats["dropped"] > 0


def test_a_large_pair(oracle):
    rng = np.random.default_rng(8)
    df, dm = bc.shared_prototypes(rng, 3000, 8192, 3000, 8)
    _, _, stats = both(oracle, df, dm, 20.0, 0.9)
    assert stats["candidates"] > 5000 and stats["matches"] > 500 and stats["lowe_fixed"] > 0 and stats["lowe_moving"] > 0


def test_planted_pairs_are_exactly_the_candidates(oracle):
    rng = np.random.default_rng(9)
    df, dm, expected = bc.spread(rng, 300, 100, 65, [0, 3, 7, 12, 19])
    f, m, d = br.candidates(df, dm, 50.0)
    assert {(int(a), int(b)): int(c) for a, b, c in zip(f, m, d)} == expected and len(expected) == 65
    got, flags, stats = both(oracle, df, dm, 50.0, 0.9)
    assert triples(got) == sorted(((f, m, float(d)) for (f, m), d in expected.items()), key=lambda t: (t[2], t[0], t[1])) and flags == 0
    # matches at the highest indices of both clouds, and in the last row of a tile, a wave and a pass
    plan = [(1299, 4999, 2), (15, 63, 3), (63, 15, 4), (1023, 511, 5), (511, 1023, 6), (1024, 0, 7)]
    df, dm, expected = bc.planted(rng, 1300, 5000, plan, floor=75)
    got, _, _ = both(oracle, df, dm, 50.0, 0.9)
    assert triples(got) == [(1299, 4999, 2.0), (15, 63, 3.0), (63, 15, 4.0), (1023, 511, 5.0), (511, 1023, 6.0), (1024, 0, 7.0)]
    df, dm = far_moving_pair(rng, 64, 16000)
    got, _, stats = both(oracle, df, dm, 32.0, 0.9)
    assert (got["moving_idx"] > 8191).any() and (got["moving_idx"] == 15999).any()
    assert stats["dropped"] >= 4 and stats["lowe_fixed"] > 0 and stats["lowe_moving"] > 0


def test_planted_refuses_an_input_it_did_not_plant():
    rng = np.random.default_rng(10)
    # random rows are ~128 bits apart: below a floor of 140 bits they are pairs nobody planted, and the generator must notice
    with pytest.raises(AssertionError):
        bc.planted(rng, 8, 8, [(0, 0, 3)], floor=140)


def test_conflict_chain_by_hand(oracle):
    for shift_f, shift_m, nf, nm in ((0, 0, 12, 12), (1088, 288, 1100, 300), (5, 0, 40, 12)):
        df, dm = bc.conflict_chain(np.random.default_rng(11), nf, nm, shift_f, shift_m)
        for max_dist in (41.0, 50.0, 80.0):
            got, flags, stats = both(oracle, df, dm, max_dist, bc.CHAIN_RATIO)
            assert triples(got) == bc.chain_expected(shift_f, shift_m) and flags == 0
            assert (stats["candidates"], stats["levels"], stats["dropped"], stats["lowe_fixed"], stats["lowe_moving"], stats["matches"]) == \
                (bc.CHAIN_CANDIDATES, bc.CHAIN_LEVELS, bc.CHAIN_DROPPED, bc.CHAIN_LOWE_FIXED, bc.CHAIN_LOWE_MOVING, 2)
        # below 40 bits the chain's indices have no larger distance left behind 20: Lowe rejects them too (:163-165)
        got, flags, _ = both(oracle, df, dm, 40.0, bc.CHAIN_RATIO)
        assert len(got) == 0 and flags == br.WARN_NO_MATCHES
        # a ratio just above 0.9f lets the 18-bit candidates through, which then block the 20-bit ones
        got, _, _ = both(oracle, df, dm, 50.0, float(np.nextafter(np.float32(0.9), np.float32(1))))
        assert triples(got) == [(bc.CHAIN_F + shift_f, 6 + shift_m, 18.0), (5 + shift_f, bc.CHAIN_M + shift_m, 18.0)]


def test_early_exit_changes_nothing(oracle):
    """three fixed rows, each with one close partner; more candidates wait at 30 bits when the last fixed row is registered: the loop
    leaves through the early exit (:138-141) and the result equals that of the same run without it"""
    rng = np.random.default_rng(12)
    plan = [dict(fixed={f: ()}, moving={f: tuple(range(f + 1)), f + 3: tuple(range(100, 130)), f + 6: tuple(range(200, 230))}) for f in range(3)]
    df, dm, expected = bc.planted(rng, 3, 10, plan)
    assert len(expected) == 9
    got, flags, stats = both(oracle, df, dm, 50.0, 0.9)
    assert stats["early_exit"] and triples(got) == [(0, 0, 1.0), (1, 1, 2.0), (2, 2, 3.0)]
    full, flags2, stats2 = br.match(df, dm, 50.0, 0.9, early_exit=False)
    assert not stats2["early_exit"] and corr_equal(got, full) and flags == flags2
    # ... and on tie-heavy clouds where the moving cloud runs out first
    for seed in range(6):
        rng = np.random.default_rng(50 + seed)
        df, dm = bc.shared_prototypes(rng, 12, 200, 10, 3)
        a = br.match(df, dm, 30.0, 1.5)
        b = br.match(df, dm, 30.0, 1.5, early_exit=False)
        assert corr_equal(a[0], b[0]) and a[1] == b[1]
        both(oracle, df, dm, 30.0, 1.5)


def test_float32_ratio_boundaries(oracle):
    df, dm, index = boundary_pair(np.random.default_rng(13))
    for ratio, pairs in RATIO_EDGES.items():
        above = float(np.nextafter(np.float32(ratio), np.float32(2)))
        at, _, stats = both(oracle, df, dm, 70.0, ratio)
        over, _, _ = both(oracle, df, dm, 70.0, above)
        assert stats["lowe_fixed"] > 0 and stats["lowe_moving"] > 0
        at, over = set(triples(at)), set(triples(over))
        for best, second in pairs:
            assert np.float32(best) / np.float32(second) == np.float32(ratio)  # the quotient EQUALS the ratio in float32 ...
            (f, m_best, m_second), (m, f_best, f_second) = index[(best, second)]
            # ... so the strict `<` rejects the best; the second best has no larger distance behind it and is rejected as well
            assert not {(f, m_best, float(best)), (f, m_second, float(second)), (f_best, m, float(best)), (f_second, m, float(second))} & at
            assert {(f, m_best, float(best)), (f_best, m, float(best))} <= over
    for ratio, expect in ((0.0, False), (1.0, True), (1.5, True)):
        got = set(triples(both(oracle, df, dm, 70.0, ratio)[0]))
        for (best, second), ((f, m_best, _), (m, f_best, _)) in index.items():
            assert ((f, m_best, float(best)) in got) == expect and ((f_best, m, float(best)) in got) == expect


def test_thresholds(oracle):
    rng = np.random.default_rng(14)
    df, dm, index = boundary_pair(rng)
    tf, tm = tie_pair(rng, 150, 140, n_base=10, flips=40)
    for max_dist in THRESHOLDS + (float("nan"),):
        got, flags, stats = both(oracle, df, dm, max_dist, 0.9)
        both(oracle, tf, tm, max_dist, 0.9)
        if not max_dist >= 1.0:  # 0, negative, NaN: no candidate at all
            assert stats["candidates"] == 0 and flags == br.WARN_NO_MATCHES
        got = set(triples(got))
        for best, second in WORD_EDGES:
            (f, m_best, _), (m, f_best, _) = index[(best, second)]
            # the second best one past the threshold is no candidate: the best stands alone in its lists and passes (:185-188);
            # one bit further it is the second best, and best / second >= 0.9
            alone = best < max_dist <= second
            assert ((f, m_best, float(best)) in got) == alone and ((f_best, m, float(best)) in got) == alone, (max_dist, best)
    # threshold 1: only identical rows
    got, _, stats = both(oracle, tf, tf[::-1].copy(), 1.0, 0.9)
    assert stats["candidates"] >= 150 and stats["levels"] == 1
    assert [bool(np.float32(255) < np.float32(t)) for t in (255.0, 255.5, 256.0)] == [False, True, True]
