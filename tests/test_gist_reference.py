"""CPU tests of tests/gist_reference.py, the restatement of BinaryGistRecognizer + PlaceRecognizer with exact k-NN that the GPU
tests hold uzl_gist_* to: against a brute-force loop, and known answers for the cases the header's contract spells out."""
import numpy as np
import pytest

from gist_reference import GistReference, brute_knn, hamming

S = 10**9


def flip(base, bits):
    d = np.array(base, np.uint8).copy()
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


Z = np.zeros(32, np.uint8)


def test_hamming_matches_bit_counting():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    b = rng.integers(0, 256, (50, 32), dtype=np.uint8)
    want = [sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, r)) for r in b]
    assert hamming(a, b).tolist() == want


@pytest.mark.parametrize("seed", range(6))
def test_knn_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    nbytes = [2, 4, 32][seed % 3]                       # short descriptors: many ties
    k = int(rng.integers(1, 12)); T = float(rng.choice([0, 3, 5.5, 10, 16, 1000]))
    g = GistReference(T=T, k_nearest_neighbors=k)
    for i in range(200):
        desc = None if rng.random() < 0.1 else rng.integers(0, 256, nbytes, dtype=np.uint8)
        g.add(desc, i * S)
        if rng.random() < 0.1 and i > 0:
            live = [p for p in range(g.count()) if g.alive[p]]
            g.remove(int(rng.choice(live)))
    for _ in range(40):
        q = rng.integers(0, 256, nbytes, dtype=np.uint8)
        pl, di = g._knn(q)
        want = brute_knn(g.desc, g.alive, q, k, T)
        assert list(zip(pl.tolist(), di.tolist())) == want


def test_ties_at_the_cutoff_go_by_place_index():
    g = GistReference(T=10, k_nearest_neighbors=3, min_time_gap=5.0)
    for i, bits in enumerate([[0, 1, 2], [5], [6, 7], [9], [12], [1, 3]]):   # distances 3, 1, 2, 1, 1, 2
        g.add(flip(Z, bits), i * 100 * S)
    res = g.search(Z, 10**6 * S)
    assert g.last_knn[0].tolist() == [1, 3, 4] and g.last_knn[1].tolist() == [1, 1, 1]
    assert res.tolist() == [1, 3, 4]
    g2 = GistReference(T=10, k_nearest_neighbors=5)
    for i, bits in enumerate([[0, 1, 2], [5], [6, 7], [9], [12], [1, 3]]):
        g2.add(flip(Z, bits), i * 100 * S)
    g2.search(Z, 10**6 * S)
    assert g2.last_knn[0].tolist() == [1, 3, 4, 2, 5] and g2.last_knn[1].tolist() == [1, 1, 1, 2, 2]


def test_recent_near_duplicates_use_up_the_k_slots():
    """the k cut of the k-NN comes before the time gap: the loop closure ranked k + 1 is not reported"""
    def run(k):
        g = GistReference(T=10, k_nearest_neighbors=k)
        g.add(flip(Z, [0, 1]), 0)                                       # the true loop closure, distance 2, 100 s ago
        for j, bits in enumerate([[], [3], [4]]):                       # near-duplicates of the last seconds, distances 0, 1, 1
            g.add(flip(Z, bits), (97 + j) * S)
        return g, g.search_and_add(Z, 100 * S)
    g, (res, pid) = run(3)
    assert pid == 4 and g.last_knn[0].tolist() == [1, 2, 3] and res.tolist() == []
    g, (res, pid) = run(4)
    assert g.last_knn[0].tolist() == [1, 2, 3, 0] and res.tolist() == [0]


@pytest.mark.parametrize("T,want", [(10, [0]), (10.5, [0]), (10.99, [0]), (11, [0, 1]), (9.99, []), (-1, [])])
def test_T_is_inclusive_and_may_be_fractional(T, want):
    g = GistReference(T=T, k_nearest_neighbors=10)
    g.add(flip(Z, range(10)), 0)
    g.add(flip(Z, range(11)), 0)
    assert g.search(Z, 100 * S).tolist() == want


def test_removed_places_are_neither_found_nor_take_a_slot():
    g = GistReference(T=10, k_nearest_neighbors=1)
    g.add(flip(Z, [0]), 0); g.add(flip(Z, [0, 1]), 0)
    g.remove(0)
    assert g.search(Z, 100 * S).tolist() == [1]
    with pytest.raises(KeyError):
        g.remove(0)
    with pytest.raises(KeyError):
        g.remove(7)


def test_nodes_without_gist_take_an_index_and_are_never_found():
    g = GistReference(T=10, k_nearest_neighbors=10)
    assert g.add(None, 0) == 0
    res, pid = g.search_and_add(None, 0)
    assert pid == 1 and res.tolist() == [] and g.last_knn[0].tolist() == []
    assert g.add(Z, 0) == 2
    assert g.search(Z, 100 * S).tolist() == [2]
    assert g.count() == 3
    g.remove(0)                                                         # a gist-less place can be removed like any other


def test_k_zero_returns_nothing():
    g = GistReference(T=10, k_nearest_neighbors=0)
    g.add(Z, 0)
    assert g.search(Z, 100 * S).tolist() == [] and g.last_knn[0].tolist() == []
    assert g.search_and_add(Z, 100 * S)[0].tolist() == []


def test_reported_once_across_search_and_search_and_add():
    g = GistReference(T=10, k_nearest_neighbors=10)
    g.add(Z, 0); g.add(flip(Z, [1]), S)
    assert g.search(Z, 100 * S, query_place=2).tolist() == [0, 1]
    assert g.search(Z, 100 * S, query_place=2).tolist() == []           # same (neighbour, query) pairs
    assert g.search(Z, 100 * S, query_place=-1).tolist() == [0, 1]
    res, pid = g.search_and_add(flip(Z, [2]), 100 * S)                   # becomes place 2: both pairs were reported
    assert pid == 2 and res.tolist() == [] and g.last_knn[0].tolist() == [0, 1]
    res, pid = g.search_and_add(flip(Z, [2]), 200 * S)
    assert res.tolist() == [2, 0, 1]


def test_descriptor_length_is_fixed_by_the_first_indexed_one():
    g = GistReference()
    g.add(None, 0)
    g.add(np.zeros(64, np.uint8), 0)
    with pytest.raises(ValueError):
        g.add(np.zeros(32, np.uint8), 0)
    with pytest.raises(ValueError):
        g.search(np.zeros(32, np.uint8), 0)
    with pytest.raises(ValueError):
        GistReference().add(np.zeros(257, np.uint8), 0)
    assert g.count() == 2
