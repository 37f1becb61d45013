"""CPU tests (no GPU needed) of tests/gfr_reference.py, the NumPy restatement of the uzl_gfr_* contract: its vectorised search,
votes and candidates against the plain-loop forms, a hand-worked scenario with known answers, and the reported-once filter."""
import numpy as np
import pytest

import gfr_reference as R

S = 10**9


@pytest.mark.parametrize("nbytes,seed", [(1, 0), (8, 1), (20, 2), (33, 3), (64, 4)])
def test_vectorised_forms_equal_the_loops(nbytes, seed):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, (6, nbytes), dtype=np.uint8)           # few distinct rows: many exact ties
    maxd = max(2, nbytes)
    r = R.GfrReference(T=2.0, k_nearest_neighbors=4, max_distance=maxd, min_time_gap=0.0)
    for node in range(12):
        rows = pool[rng.integers(0, 6, 9)].copy()
        for i in range(9):
            for b in rng.integers(0, 8 * nbytes, int(rng.integers(0, 3))):
                rows[i, b // 8] ^= np.uint8(1 << (b % 8))
        features = [r.get_feature(f)[0] for f in range(r.F)]
        links = [list(x) for x in r.links]
        want_m, want_v = R.brute_votes(features, links, rows, maxd, r.count())
        r.search_and_add(rows, node * S)
        assert [(int(f), int(d)) for f, d in zip(*r.last_matches)] == want_m
        assert r.last_votes.tolist() == want_v
        assert R.candidates(np.array(want_v), 2.0) == R.brute_candidates(want_v, 2.0)
    assert r.F > 6 and r.counters["vote_ties"] > 0 and r.counters["duplicate_links"] > 0


BASE = [0x00, 0x03, 0x05, 0x06, 0x09, 0x0A, 0x0C, 0x0F, 0x11, 0x12, 0x14]     # even parity: pairwise distance >= 2


def rows_of(lows, high=0x7F):
    return np.array([[high, lo] for lo in lows], np.uint8)


def test_hand_worked_scenario():
    """2-byte rows (the popcount rule wants more than 6 set bits), max_distance = 2 (a row matches at distance 0 or 1), T = 10.5
    (acts as 11), k = 0 (one neighbour gets through), min_time_gap = 5 s, one node every 10 s."""
    r = R.GfrReference(T=10.5, k_nearest_neighbors=0, max_distance=2, min_time_gap=5.0)
    # node 0: eleven features and a row with exactly 3 * bytes = 6 set bits, which is dropped
    nb, p = r.search_and_add(np.concatenate([rows_of(BASE), np.array([[0x00, 0x3F]], np.uint8)]), 0)
    assert (nb.tolist(), p, r.F, r.link_count()) == ([], 0, 11, 11) and r.counters["popcount_drops"] == 1
    assert r.last_matches[0].tolist() == [-1] * 12 and r.last_matches[1].tolist() == [-1] * 12     # F was 0
    # node 1: every row one bit off its feature: matched at distance 1, eleven votes for place 0
    nb, p = r.search_and_add(rows_of(BASE, 0x7E), 10 * S)
    assert (nb.tolist(), p, r.F, r.link_count()) == ([0], 1, 11, 22)
    assert r.last_matches[0].tolist() == list(range(11)) and r.last_matches[1].tolist() == [1] * 11
    assert r.last_votes.tolist() == [11, 0]
    # node 2: ten rows, ten votes each for places 0 and 1: below T = 10.5
    nb, p = r.search_and_add(rows_of(BASE[:10]), 20 * S)
    assert (nb.tolist(), p, r.link_count()) == ([], 2, 32) and r.last_votes.tolist() == [10, 10, 0]
    # node 3: nine features, the first of them three times: 9 + 2 = 11 votes each for places 0, 1, 2; a three-way tie goes to
    # the lower place, and k = 0 stops after the first
    nb, p = r.search_and_add(rows_of(BASE[:9] + [BASE[0], BASE[0]]), 30 * S)
    assert (nb.tolist(), p, r.link_count()) == ([0], 3, 43) and r.last_votes.tolist() == [11, 11, 11, 0]
    assert r.get_feature(0)[1].tolist() == [0, 1, 2, 3, 3, 3] and r.counters["duplicate_links"] == 2
    # a search with feature 0 four times: place 3 is linked three times and collects 12 votes, the others 4
    nb = r.search(rows_of([BASE[0]] * 4), 40 * S)
    assert nb.tolist() == [3] and r.last_votes.tolist() == [4, 4, 4, 12, 0]
    assert r.link_count() == 43 and r.count() == 4
    # place 0 is removed: it still collects votes, and is dropped before the k count
    r.remove(0)
    nb, p = r.search_and_add(rows_of(BASE), 40 * S)
    assert r.last_votes.tolist() == [11, 11, 10, 11, 0] and (nb.tolist(), p, r.link_count()) == ([1], 4, 54)
    # node 5 comes with another feature type: the repository restarts, place indices go on
    nb, p = r.search_and_add(rows_of(BASE), 50 * S, feature_type=3)
    assert (nb.tolist(), p, r.F, r.link_count()) == ([], 5, 11, 11)
    assert r.last_votes.tolist() == [0] * 6 and r.last_matches[1].tolist() == [-1] * 11
    assert r.search(rows_of(BASE), 60 * S, feature_type=3).tolist() == [5] and r.last_votes.tolist() == [0, 0, 0, 0, 0, 11, 0]
    # ... and a search with the old type clears it again
    assert r.search(rows_of(BASE), 60 * S, feature_type=2).tolist() == [] and r.F == 0 and r.bytes is None
    with pytest.raises(KeyError):
        r.remove(0)


def test_reported_once_filter():
    r = R.GfrReference(T=2.0, k_nearest_neighbors=10, max_distance=2, min_time_gap=5.0)
    for i in range(3):
        assert r.add(rows_of(BASE[:4]), i * 10 * S) == i
    q = rows_of(BASE[:4])
    assert r.search(q, 100 * S, query_place=7).tolist() == [0, 1, 2]          # 4 votes each, place order
    assert r.search(q, 100 * S, query_place=7).tolist() == []                 # every (neighbour, 7) pair was reported
    assert r.search(q, 100 * S, query_place=8).tolist() == [0, 1, 2]          # another querying place
    assert r.search(q, 22 * S, query_place=9).tolist() == [0, 1]              # place 2 is 2 s away
    assert r.search(q, 100 * S, query_place=9).tolist() == [2]                # ... the other two were reported to 9
    nb, p = r.search_and_add(q, 100 * S)
    assert (nb.tolist(), p) == ([0, 1, 2], 3)
    assert r.search(q, 200 * S, query_place=3).tolist() == [3]                # (0, 3), (1, 3), (2, 3) are known
    assert r.counters["neighbours"] == 13
    # no live place: nothing is returned and nothing is touched, not even the type
    e = R.GfrReference()
    assert e.search(q, 0, feature_type=5).tolist() == [] and e.type == -1
    e.add(None, 0); e.remove(0)
    assert e.search(q, 0, feature_type=5).tolist() == [] and e.type == -1 and e.count() == 1
