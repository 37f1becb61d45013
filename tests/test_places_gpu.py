"""uzl_places_* on the device against the restatement (tests/places_reference.py) and the CPU checker after every call: neighbours,
place index, count() and last_counts over the earlier places (a search_and_add's own slot is left out: the device counts before
it inserts).  Everything is integer-exact.  Cases: every key width, wide descriptors, every configuration field off its default,
the output cap, the all-ones and all-zero keys across a table rebuild, growth with removes, hub keys, degenerate calls, two handles,
bad arguments."""
import ctypes as C

import numpy as np
import pytest

import places_scenes as PS
from places_reference import PlacesReference, keys_of, popcount

pytestmark = pytest.mark.gpu
S = PS.S


def trio(capi, oracle, **cfg):
    return {"reference": PlacesReference(**cfg), "oracle": oracle.Places(**cfg), "device": capi.Places(**cfg)}


def close(impls):
    impls["oracle"].close(); impls["device"].close()


def rnd(rng, rows, nbytes=32):
    return rng.integers(0, 256, (rows, nbytes), dtype=np.uint8)


def dense_keys(desc, key_width=8):
    """number of a frame's keys that pass search_and_add's popcount rule"""
    return sum(popcount(k) > 3 * key_width for row in keys_of(desc, key_width) for k in row)


@pytest.mark.parametrize("key_width", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_key_width(capi, oracle, key_width):
    """36 frames of 64 to 400 rows (and the sizes around min_rows_to_add), all four operations mixed.  Key widths 1, 2 and 3 have
    32, 16 and 10 tables; every one of them counts, and the similarity divides by their number."""
    ops = PS.mixed_sequence(200 + key_width, key_width, n_calls=36, rows_lo=64, rows_hi=400)
    impls = trio(capi, oracle, key_width=key_width, **PS.CFG)
    out = PS.run(impls, ops)
    assert out["neighbours"] >= 10 and impls["reference"].kept > 100 and impls["reference"].skipped > 100
    close(impls)


@pytest.mark.parametrize("key_width,nbytes", [(8, 64), (8, 40), (3, 64), (5, 40)])
def test_wide_descriptors(capi, oracle, key_width, nbytes):
    """BRISK-512 rows are 64 bytes: the row stride is `bytes`, the keys come from the first 32, and the bytes from 32 up influence
    nothing - the same sequence with other bytes there gives the same output"""
    a = PS.mixed_sequence(300 + nbytes, key_width, nbytes, n_calls=24, tail_seed=1)
    b = PS.mixed_sequence(300 + nbytes, key_width, nbytes, n_calls=24, tail_seed=2)
    assert any(not np.array_equal(x[1][:, 32:], y[1][:, 32:]) for x, y in zip(a, b) if x[0] != "remove" and len(x[1]))
    impls = trio(capi, oracle, key_width=key_width, **PS.CFG)
    out = PS.run(impls, a)
    assert out["neighbours"] >= 5
    other = capi.Places(key_width=key_width, **PS.CFG); own = PS.OwnSlot()
    for i, op in enumerate(b):
        r = PS.apply(other, op)
        assert r["nb"] == out["calls"][i]["nb"] and r["idx"] == out["calls"][i]["idx"], i
        assert np.array_equal(own.hide(op[0], r["counts"]), out["calls"][i]["counts"]), i
    other.close(); close(impls)


def sharing(rng, base_row, rows, key_width, n_keys=1):
    """`rows` random rows that share exactly the first n_keys keys with base_row (the byte after them is made to differ)"""
    d = rnd(rng, rows, len(base_row))
    d[:, :n_keys * key_width] = base_row[:n_keys * key_width]
    d[:, n_keys * key_width] = base_row[n_keys * key_width] ^ 0x5A
    return d


@pytest.mark.parametrize("key_width,count,below", [(8, 10, 9), (3, 7, 6), (1, 48, 47)])
def test_threshold_on_the_boundary(capi, oracle, key_width, count, below):
    """T equal to float32(count) / float32(tables): that count is a neighbour, one collision fewer is not"""
    rng = np.random.default_rng(key_width)
    nt = len(range(0, 32 - key_width + 1, key_width))
    T = float(np.float32(count) / np.float32(nt))
    base = rnd(rng, 1)[0]
    if key_width == 1:
        # with one-byte keys random rows collide everywhere: count collisions of constant rows instead.  A stored row of 32 bytes
        # 0xC3 meets a query row of 0xC3 in all 32 tables; a query row with 16 (15) bytes 0xC3 and the rest 0x3C in 16 (15)
        base = np.full(32, 0xC3, np.uint8)
        def query(c):
            q = np.full((2, 32), 0x3C, np.uint8); q[0] = 0xC3; q[1, :c - 32] = 0xC3
            return q
    else:
        def query(c):
            return sharing(rng, base, c, key_width)
    impls = trio(capi, oracle, key_width=key_width, T=T, min_rows_to_add=0)
    ops = [("add", base[None, :], 0), ("search", query(count), 100 * S, -1), ("search", query(below), 100 * S, -2),
           ("search", query(count), 100 * S, -3)]
    out = PS.run(impls, ops)
    assert [c["nb"] for c in out["calls"][1:]] == [[0], [], [0]]
    assert [int(c["counts"][0]) for c in out["calls"][1:]] == [count, below, count]
    close(impls)


@pytest.mark.parametrize("k", [1, 0, 2])
def test_k_nearest_neighbors(capi, oracle, k):
    """k = 1 reports the best survivor of the time filter only.  k = 0 is accepted and behaves as k = 1: the walk stops after the
    survivor that makes the number of survivors reach k, and it tests that only after taking one."""
    rng = np.random.default_rng(40 + k)
    base = rnd(rng, 30)
    impls = trio(capi, oracle, k_nearest_neighbors=k, T=1.0, min_rows_to_add=0)
    ops = [("add", base[:10 + 5 * i], i * S) for i in range(4)]              # place i shares 10 + 5 i rows with the query
    ops += [("search", base, 3 * S + 5 * S + 1, -1),                          # place 3 is 5 s + 1 ns away, the others further
            ("search", base, 3 * S + 5 * S, -2),                              # place 3 exactly 5 s: dropped before the k cut
            ("search_and_add", base, 100 * S)]
    out = PS.run(impls, ops)
    kk = max(k, 1)
    assert [c["nb"] for c in out["calls"][4:]] == [[3, 2][:kk], [2, 1][:kk], [3, 2][:kk]]
    assert list(out["calls"][4]["counts"]) == [40, 60, 80, 100]
    close(impls)


def test_min_rows_to_add(capi, oracle):
    """0: a one-row frame is indexed, a frame without rows is not.  At `rows`: a frame of exactly that many rows is matched but not
    indexed, one more row and it is."""
    rng = np.random.default_rng(50)
    for min_rows, sizes in ((0, (0, 1)), (70, (70, 71))):
        impls = trio(capi, oracle, min_rows_to_add=min_rows, T=0.25, min_time_gap=0.0)
        f = [rnd(rng, n) for n in sizes for _ in range(2)]
        ops = [("search_and_add", f[0], 1 * S), ("add", f[1], 2 * S), ("search_and_add", f[2], 3 * S), ("add", f[3], 4 * S)]
        ops += [("search", np.concatenate(f), 10 * S, -1), ("search_and_add", np.concatenate(f), 11 * S)]
        out = PS.run(impls, ops)
        # every row of an indexed frame meets itself in 4 tables; search_and_add indexes, and matches, only the dense keys
        want = [0, 0, dense_keys(f[2]), sizes[1] * 4]
        assert list(out["calls"][4]["counts"]) == want
        assert out["calls"][4]["nb"] == sorted((p for p in (2, 3) if want[p]), key=lambda p: (-want[p], p)) and want[3]
        assert list(out["calls"][5]["counts"][:4]) == [0, 0, dense_keys(f[2]), dense_keys(f[3])]
        close(impls)


def test_time_gap_zero_and_epoch_stamps(capi, oracle):
    """min_time_gap 0: a place at the same nanosecond is dropped (strict >), one 1 ns away is reported.  Stamps of about 1.7e18 ns
    with gaps of min_time_gap +- 1 us (and +- 1 ns): the difference is taken on the integers; doubles of that size are 256 ns apart"""
    rng = np.random.default_rng(60)
    base = 1_700_000_000 * S + 123_456_789
    d = rnd(rng, 20)
    impls = trio(capi, oracle, min_time_gap=0.0, T=1.0, min_rows_to_add=0)
    out = PS.run(impls, [("add", d, base), ("add", d, base + 1), ("search", d, base, -1), ("search", d, base + 1, -2)])
    assert [c["nb"] for c in out["calls"][2:]] == [[1], [0]]
    close(impls)
    for eps in (1000, 1):
        impls = trio(capi, oracle, min_time_gap=5.0, T=1.0, min_rows_to_add=0)
        ops = [("add", d, base), ("add", d, base + 10 * S)]
        # a query 5 s + eps after place 0 is 5 s - eps before place 1
        ops += [("search", d, base + 5 * S + eps, -1), ("search", d, base + 5 * S - eps, -2), ("search", d, base + 5 * S, -3),
                ("search_and_add", d, base + 15 * S + eps), ("search_and_add", d, base + 15 * S - eps)]
        out = PS.run(impls, ops)
        assert [c["nb"] for c in out["calls"][2:]] == [[0], [1], [], [0, 1], [0]], eps
        close(impls)


def test_output_cap(capi, oracle):
    """*n_neighbors is the full number, only the first cap are written, and the pairs beyond cap count as reported"""
    rng = np.random.default_rng(70)
    base = rnd(rng, 60)
    L = capi.lib()
    for cap in (0, 1):
        ref = PlacesReference(T=1.0, min_rows_to_add=0); g = capi.Places(T=1.0, min_rows_to_add=0); o = oracle.Places(T=1.0, min_rows_to_add=0)
        for i in range(5):
            for impl in (ref, g, o):
                impl.add(base[:20 + 8 * i], i * S)                             # best match: place 4
        want_all = [4, 3, 2, 1, 0]

        def search(desc, query_place, cap, null=False):
            out = np.full(8, -7, np.int32); n = C.c_int32(-1)
            rc = L.uzl_places_search(g._h, desc.ctypes.data_as(capi.c_u8p), C.c_int32(len(desc)), C.c_int32(32), C.c_int64(100 * S),
                                     C.c_int32(query_place), C.c_int32(cap), None if null else out.ctypes.data_as(capi.c_i32p), C.byref(n))
            assert rc == capi.UZL_OK
            return n.value, list(out)

        n, out = search(base, 3, cap, null=(cap == 0))
        assert n == 5 and out == want_all[:cap] + [-7] * (8 - cap)
        assert list(ref.search(base, 100 * S, query_place=3, cap=cap)) == want_all[:cap] and ref.last_n == 5
        assert list(o.search(base, 100 * S, query_place=3, cap=cap)) == want_all[:cap]
        n, out = search(base, 3, 8)                                            # the same query place again: nothing is new
        assert n == 0 and out == [-7] * 8 and len(ref.search(base, 100 * S, query_place=3)) == 0 and len(o.search(base, 100 * S, query_place=3)) == 0
        n, out = search(base, 2, 8)                                            # another one: all five
        assert n == 5 and out[:5] == want_all
        # search_and_add with the same cap
        out = np.full(8, -7, np.int32); n = C.c_int32(-1); idx = C.c_int32(-1)
        rc = L.uzl_places_search_and_add(g._h, base.ctypes.data_as(capi.c_u8p), C.c_int32(60), C.c_int32(32), C.c_int64(200 * S), C.c_int32(cap),
                                         out.ctypes.data_as(capi.c_i32p), C.byref(n), C.byref(idx))
        assert rc == capi.UZL_OK and (n.value, idx.value) == (5, 5) and list(out) == want_all[:cap] + [-7] * (8 - cap)
        nb, pid = ref.search_and_add(base, 200 * S, cap=cap)
        assert (list(nb), pid, ref.last_n) == (want_all[:cap], 5, 5)
        assert len(g.search(base, 200 * S, query_place=5)) == 0 == len(ref.search(base, 200 * S, query_place=5))
        assert np.array_equal(g.last_counts(), ref.last_counts())
        g.close(); o.close()


def test_growth_with_history_and_the_reserved_keys(capi, oracle):
    """40 adds of 1000 random rows pass half of the initial 65536 slots per table and the 65536-entry arena (about 40 000 rows in
    all).  Before that: rows of 0xFF (the all-ones key is the tables' empty marker and lives in an extra slot) and rows of 0x00
    (add and search take the key, search_and_add's popcount rule skips it), and removes.  After it: the same counts as before, 0 for
    the removed places, the others exact; then the 0xFF place is removed and matched again."""
    rng = np.random.default_rng(80)
    ones = rnd(rng, 200); ones[:50] = 0xFF
    zeros = rnd(rng, 200); zeros[:30] = 0x00
    zeros2 = rnd(rng, 200); zeros2[:20] = 0x00
    q_ones = np.full((3, 32), 0xFF, np.uint8); q_zero = np.zeros((2, 32), np.uint8)
    big = [rnd(rng, 1000) for _ in range(40)]
    ops = [("search_and_add", ones, 0), ("add", zeros, 1 * S), ("search_and_add", zeros2, 2 * S),
           ("search", q_ones, 50 * S, -1), ("search", q_zero, 50 * S, -2)]
    removed = [5, 9, 14]                                                       # places 3 + i hold big[i]
    for i, f in enumerate(big):
        ops.append(("add", f, (100 + i) * S))
        if 3 + i in removed:
            ops.append(("remove", 3 + i, f))
    n_before = len(ops)
    probe = np.concatenate([big[0][:100], big[2][:100], big[7][:100], big[11][:100], big[30][:100], big[39][:100]])
    ops += [("search", q_ones, 900 * S, -3), ("search", q_zero, 900 * S, -4), ("search", probe, 900 * S, -5),
            ("remove", 0, ones), ("search", q_ones, 900 * S, -6), ("remove", 1, zeros), ("search", q_zero, 900 * S, -7),
            ("search_and_add", np.concatenate([q_ones, big[20][:200]]), 901 * S), ("search", q_ones, 950 * S, -8)]
    impls = trio(capi, oracle, T=1.0, k_nearest_neighbors=4)
    out = PS.run(impls, ops)
    c = out["calls"]
    assert c[3]["counts"][0] == 3 * 50 * 4 and c[4]["counts"][1] == 2 * 30 * 4 and c[4]["counts"][2] == 0
    assert c[3]["nb"] == [0] and c[4]["nb"] == [1]
    a = c[n_before:]
    assert a[0]["counts"][0] == 600 and a[1]["counts"][1] == 240 and a[1]["counts"][2] == 0
    want = np.zeros(43, np.int64); want[[3, 10, 33, 42]] = 400                 # places 5 and 14 (big[2], big[11]) were removed
    assert np.array_equal(a[2]["counts"], want) and a[2]["nb"] == [3, 10, 33, 42]
    assert not a[4]["counts"].any() and a[4]["nb"] == [] and not a[6]["counts"].any()
    assert a[7]["idx"] == 43 and a[7]["counts"][23] == dense_keys(big[20][:200]) > 700 and a[7]["nb"] == [23]
    assert a[8]["counts"][43] == 9 * 4 and a[8]["nb"] == [43]                  # the all-ones key again, inserted after the rebuild
    close(impls)


def test_hub_key(capi, oracle):
    """one key under which every row of 30 places is listed (600 entries): many lanes walk the same list and add to the same counters"""
    rng = np.random.default_rng(90)
    hub = rnd(rng, 1)[0]; hub[:8] = 0xEE
    impls = trio(capi, oracle, T=1.0, min_rows_to_add=0, k_nearest_neighbors=3)
    ops = []
    for i in range(30):
        ops.append(("search_and_add" if i % 2 else "add", sharing(rng, hub, 20, 8), i * S))
    ops.append(("search", sharing(rng, hub, 256, 8), 1000 * S, -1))
    ops.append(("remove", 7, ops[7][1])); ops.append(("remove", 8, ops[8][1][:5]))       # 5 of 8's rows name the hub key: all 20 entries go
    ops.append(("search", sharing(rng, hub, 300, 8), 1000 * S, -2))
    out = PS.run(impls, ops)
    for i in range(1, 30, 2):
        assert list(out["calls"][i]["counts"][:i]) == [400] * i, i               # 20 rows x 20 entries per earlier place
    assert list(out["calls"][30]["counts"]) == [256 * 20] * 30 and out["calls"][30]["nb"] == [0, 1, 2]
    want = [300 * 20] * 30; want[7] = want[8] = 0
    assert list(out["calls"][33]["counts"]) == want and out["calls"][33]["nb"] == [0, 1, 2]
    close(impls)


def test_degenerate_calls(capi, oracle):
    rng = np.random.default_rng(100)
    none = np.zeros((0, 32), np.uint8)
    f = rnd(rng, 50); small = f[:10]
    impls = trio(capi, oracle, T=1.0, min_rows_to_add=10, min_time_gap=0.0)
    ops = [("search", f, 0, -1), ("search", none, 0, -1), ("remove", 0, f), ("remove", -1, f),        # on an empty handle
           ("search_and_add", none, 1 * S), ("add", none, 2 * S), ("add", f, 3 * S), ("search_and_add", small, 4 * S),
           ("search", none, 10 * S, -1), ("search", f, 10 * S, -1),
           ("remove", 3, small),                                                  # a place too small to have been indexed
           ("remove", 0, none), ("remove", 0, f),                                 # with no rows; again: already removed
           ("remove", 99, f), ("remove", -3, f), ("remove", 2**31 - 1, f),        # unknown ids; place 2's entries stay
           ("search", f, 10 * S, -2), ("remove", 2, none), ("search", f, 10 * S, -3), ("search_and_add", f, 11 * S)]
    out = PS.run(impls, ops)
    c = out["calls"]
    assert c[0]["nb"] == [] and len(c[0]["counts"]) == 0 and c[3]["count"] == 0
    assert c[7]["nb"] == [2] and list(c[7]["counts"][:3]) == [0, 0, 40]
    assert list(c[8]["counts"]) == [0, 0, 0, 0] and list(c[9]["counts"]) == [0, 0, 200, 0] and c[9]["nb"] == [2]
    assert list(c[16]["counts"]) == [0, 0, 200, 0] and c[16]["nb"] == [2]
    assert list(c[18]["counts"]) == [0, 0, 200, 0] and c[18]["nb"] == []          # removed without rows: still counted, never reported
    assert c[19]["idx"] == 4 and c[19]["nb"] == []
    close(impls)


def test_two_handles_alternately(capi, oracle):
    a = PS.mixed_sequence(7, 2, n_calls=20); b = PS.mixed_sequence(8, 8, 64, n_calls=20)
    A = trio(capi, oracle, key_width=2, **PS.CFG); B = trio(capi, oracle, key_width=8, T=1.0, k_nearest_neighbors=5, min_rows_to_add=40)
    n = 0
    ra, rb = PS.Runner(A), PS.Runner(B)
    for i in range(max(len(a), len(b))):
        if i < len(a):
            n += ra.run(a[i:i + 1])["neighbours"]
        if i < len(b):
            n += rb.run(b[i:i + 1])["neighbours"]
    assert n >= 10
    close(A); close(B)


def test_bad_arguments(capi):
    L = capi.lib()
    for bad in (dict(key_width=0), dict(key_width=9), dict(key_width=-1), dict(min_time_gap=-1.0), dict(min_time_gap=-1e-9)):
        with pytest.raises(capi.UzlError) as e:
            capi.Places(**bad)
        assert e.value.status == capi.UZL_ERR_BAD_ARG, bad
    g = capi.Places(min_rows_to_add=0, T=1.0)
    d = np.full((4, 32), 0xF0, np.uint8)
    for call in (lambda: g.add(np.zeros((4, 31), np.uint8), 0), lambda: g.search_and_add(np.zeros((4, 16), np.uint8), 0),
                 lambda: g.search(np.zeros((4, 8), np.uint8), 0), lambda: g.remove(0, np.zeros((4, 31), np.uint8))):
        with pytest.raises(capi.UzlError) as e:
            call()
        assert e.value.status == capi.UZL_ERR_BAD_ARG
    assert g.count() == 0
    p8 = d.ctypes.data_as(capi.c_u8p); out = np.zeros(4, np.int32); n = C.c_int32(); idx = C.c_int32()
    args = (p8, C.c_int32(4), C.c_int32(32), C.c_int64(0))
    assert L.uzl_places_search_and_add(g._h, *args, C.c_int32(4), out.ctypes.data_as(capi.c_i32p), None, C.byref(idx)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_places_search_and_add(g._h, *args, C.c_int32(4), None, C.byref(n), C.byref(idx)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_places_search_and_add(g._h, *args, C.c_int32(-1), out.ctypes.data_as(capi.c_i32p), C.byref(n), C.byref(idx)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_places_search_and_add(g._h, None, C.c_int32(4), C.c_int32(32), C.c_int64(0), C.c_int32(4), out.ctypes.data_as(capi.c_i32p),
                                       C.byref(n), C.byref(idx)) == capi.UZL_ERR_BAD_ARG
    assert g.count() == 0                                                      # a refused call adds no place
    assert L.uzl_places_search_and_add(g._h, *args, C.c_int32(4), out.ctypes.data_as(capi.c_i32p), C.byref(n), None) == capi.UZL_OK   # place_index is optional
    assert L.uzl_places_add(g._h, *args, None) == capi.UZL_OK
    assert L.uzl_places_search(g._h, *args, C.c_int32(-1), C.c_int32(4), out.ctypes.data_as(capi.c_i32p), None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_places_search(g._h, *args, C.c_int32(-1), C.c_int32(4), None, C.byref(n)) == capi.UZL_ERR_BAD_ARG
    # the handle still works
    assert g.count() == 2 and list(g.search(d, 100 * S)) == [0, 1] and list(g.last_counts()) == [64, 64]
    g.close()
