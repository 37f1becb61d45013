"""tests/places_reference.py (the plain-Python restatement of the uzl_places_* contract) against the CPU checker, call by call, for
every key width and for 32- and 64-byte descriptors, plus scenarios small enough to count on paper (CPU)."""
import numpy as np
import pytest

import places_scenes as PS
from places_reference import PlacesReference, keys_of, num_tables, popcount

S = PS.S


def test_number_of_tables(oracle):
    """FastLshSet::clear: one table per byte offset 0, kw, 2 kw, ... < 32 - kw + 1"""
    want = {1: 32, 2: 16, 3: 10, 4: 8, 5: 6, 6: 5, 7: 4, 8: 4}
    for kw, nt in want.items():
        assert num_tables(kw) == nt and PlacesReference(key_width=kw).num_tables() == nt
        o = oracle.Places(key_width=kw)
        assert o.num_tables() == nt
        o.close()
        row = np.arange(40, dtype=np.uint8).reshape(1, 40)
        keys = keys_of(row, kw)[0]
        assert len(keys) == nt and keys[-1] == int.from_bytes(bytes(range((nt - 1) * kw, nt * kw)), "little")


def test_hand_worked_scenario(oracle):
    """key_width 4 (8 tables), min_rows_to_add 2, T 1.0, k 2, min_time_gap 1 s.  Rows are 32 equal bytes, so a row of byte b has
    the key b b b b in all 8 tables: popcount 4 popcount(b), to be > 12."""
    def rows(*b):
        return np.repeat(np.array(b, np.uint8)[:, None], 32, axis=1)

    for impl in (PlacesReference(key_width=4, min_rows_to_add=2, T=1.0, k_nearest_neighbors=2, min_time_gap=1.0),
                 oracle.Places(key_width=4, min_rows_to_add=2, T=1.0, k_nearest_neighbors=2, min_time_gap=1.0)):
        # place 0: rows FF, FF, 0F, 01.  FF (32 bits) and 0F (16 bits) pass the popcount rule, 01 (4 bits) does not.
        # own slot: the second FF row meets the first in 8 tables
        nb, idx = impl.search_and_add(rows(0xFF, 0xFF, 0x0F, 0x01), 10 * S)
        assert (list(nb), idx, list(impl.last_counts())) == ([], 0, [8])
        # place 1 by add(): unfiltered, so 01 is indexed here.  3 rows
        assert impl.add(rows(0x01, 0x0F, 0x55), 11 * S) == 1
        # place 2: two rows only, not more than min_rows_to_add -> matched unfiltered, not indexed.
        # FF meets place 0 twice per table: 16.  01 meets place 1 once per table: 8.
        nb, idx = impl.search_and_add(rows(0xFF, 0x01), 20 * S)
        assert (list(nb), idx, list(impl.last_counts())) == ([0, 1], 2, [16, 8, 0])
        # place 3: rows 0F, 0F, 01 are indexed with the filter: 0F meets place 0 (one entry) and place 1 (one entry) in 8 tables, twice
        # = 16 each; 01 is skipped, so place 1 gets nothing more; the second 0F meets the first: own slot 8.
        # Equal similarities: lower index first.  Place 2 was never indexed.
        nb, idx = impl.search_and_add(rows(0x0F, 0x0F, 0x01), 30 * S)
        assert (list(nb), idx, list(impl.last_counts())) == ([0, 1], 3, [16, 16, 0, 8])
        # search: unfiltered; 0F now meets places 0, 1 and 3 (twice): 8, 8, 16.  k = 2 keeps 3 and 0.  20.5 s is 0.5 s from no place.
        nb = impl.search(rows(0x0F), 20 * S + S // 2, query_place=-1)
        assert (list(nb), list(impl.last_counts())) == ([3, 0], [8, 8, 0, 16])
        # the same search again: both pairs were reported for query place -1; place 1 is beyond the k cut, not reported either
        assert list(impl.search(rows(0x0F), 20 * S + S // 2, query_place=-1)) == []
        # for query place 2 the pair (0, 2) was reported when place 2 was added: only 3 is new
        assert list(impl.search(rows(0x0F), 20 * S + S // 2, query_place=2)) == [3]
        # another query place: reported again.  At 30.5 s place 3 is only 0.5 s away: dropped before the k cut, so 0 and 1 remain
        assert list(impl.search(rows(0x0F), 30 * S + S // 2, query_place=1)) == [0, 1]
        # remove place 3 with its rows: its 0F entries go, and it is dead
        impl.remove(3, rows(0x0F, 0x0F, 0x01))
        nb = impl.search(rows(0x0F), 50 * S, query_place=-4)
        assert (list(nb), list(impl.last_counts())) == ([0, 1], [8, 8, 0, 0])
        impl.remove(3, rows(0x0F)); impl.remove(-1, rows(0x0F)); impl.remove(17, rows(0x0F))       # no-ops
        assert list(impl.search(rows(0x0F), 50 * S, query_place=-2)) == [0, 1] and impl.count() == 4
        # removing with only part of the rows leaves the other entries counted, but the place is dead: never reported
        impl.remove(0, rows(0x0F))
        nb = impl.search(rows(0xFF, 0x0F), 50 * S, query_place=-3)
        assert (list(nb), list(impl.last_counts())) == ([1], [16, 8, 0, 0])


def test_threshold_is_inclusive(oracle):
    """similarity = float32(count) / float32(tables) >= T, at key_width 3 (10 tables) with 7 collisions: T equal to the float32
    quotient keeps the place, the next double above does not - and neither does the double 0.7, which is above float32(0.7)"""
    row = np.zeros((1, 32), np.uint8); row[0, :21] = 0xFF           # the first 7 of the 10 three-byte keys are FF FF FF, the others 0
    q = np.full((1, 32), 0x11, np.uint8); q[0, :21] = 0xFF          # shares exactly those 7
    t_eq = float(np.float32(7) / np.float32(10))
    for T, want in ((t_eq, [0]), (np.nextafter(t_eq, 1.0), []), (0.7, [])):
        for impl in (PlacesReference(key_width=3, min_rows_to_add=0, T=T), oracle.Places(key_width=3, min_rows_to_add=0, T=T)):
            impl.add(row, 0)
            assert list(impl.search(q, 100 * S)) == want and list(impl.last_counts()) == [7]


@pytest.mark.parametrize("nbytes", [32, 64])
@pytest.mark.parametrize("key_width", [1, 2, 3, 4, 5, 6, 7, 8])
def test_reference_equals_oracle(oracle, key_width, nbytes):
    ops = PS.mixed_sequence(100 + key_width, key_width, nbytes)
    ref = PlacesReference(key_width=key_width, **PS.CFG); o = oracle.Places(key_width=key_width, **PS.CFG)
    out = PS.run({"reference": ref, "oracle": o}, ops, own_slot=True)
    o.close()
    kinds = [op[0] for op in ops]
    assert all(kinds.count(k) >= 3 for k in ("search_and_add", "add", "search", "remove"))
    assert out["neighbours"] >= 10                                   # the case reports neighbours ...
    assert ref.kept > 100 and ref.skipped > 100                      # ... and sees both sides of matchAndAdd's popcount rule
    sizes = {len(op[1]) for op in ops if op[0] in ("search_and_add", "add")}
    assert {0, 1, PS.CFG["min_rows_to_add"], PS.CFG["min_rows_to_add"] + 1} <= sizes
    # frames of exactly min_rows_to_add rows are not indexed, one row more is: a later search with those rows tells them apart
    for i, op in enumerate(ops):
        if op[0] == "add" and len(op[1]) in (PS.CFG["min_rows_to_add"], PS.CFG["min_rows_to_add"] + 1):
            place = out["calls"][i]["idx"]
            ref.search(op[1], 10**6 * S)
            if ref.alive[place]:
                assert (ref.last_counts()[place] > 0) == (len(op[1]) > PS.CFG["min_rows_to_add"])


def test_bytes_from_32_up_are_ignored():
    a = PS.mixed_sequence(5, 8, 64, tail_seed=1); b = PS.mixed_sequence(5, 8, 64, tail_seed=2)
    assert any(not np.array_equal(x[1], y[1]) for x, y in zip(a, b) if x[0] != "remove")
    assert all(np.array_equal(x[1][:, :32], y[1][:, :32]) for x, y in zip(a, b) if x[0] != "remove" and len(x[1]))
    ra, rb = PlacesReference(key_width=8, **PS.CFG), PlacesReference(key_width=8, **PS.CFG)
    for x, y in zip(a, b):
        u, v = PS.apply(ra, x), PS.apply(rb, y)
        assert u["nb"] == v["nb"] and np.array_equal(u["counts"], v["counts"])


def test_popcount_rule_boundary():
    """strictly more than 3 key_width set bits"""
    for kw in (1, 5, 8):
        key = np.zeros((1, 32), np.uint8)
        bits = 3 * kw
        key[0, :bits // 8] = 0xFF
        if bits % 8:
            key[0, bits // 8] = (1 << (bits % 8)) - 1
        assert popcount(keys_of(key, kw)[0][0]) == 3 * kw
        r = PlacesReference(key_width=kw, min_rows_to_add=0, T=0.0)
        r.search_and_add(key, 0)
        assert r.kept == 0 and not r.tables[0]
        key[0, kw - 1] |= 0x80
        r.search_and_add(key, 0)
        assert r.tables[0] and popcount(keys_of(key, kw)[0][0]) == 3 * kw + 1
