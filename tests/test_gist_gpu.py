"""GPU tests of uzl_gist_* (BinaryGistRecognizer + PlaceRecognizer with exact k-NN): every call of randomized sequences equals the
CPU restatement tests/gist_reference.py exactly (neighbours, place indices, the k-NN list before the filters); the batch forms
equal the same nodes fed one at a time; bad arguments return their codes and leave the handle as it was."""
import ctypes as C

import numpy as np
import pytest

from gist_reference import GistReference

S = 10**9
pytestmark = pytest.mark.gpu


def trajectory(rng, n, nbytes, base=None, revisit=0.15, t0=0):
    """descriptors of a camera run: each frame a few bits off the previous one (near-duplicates of the last seconds), now and then
    a revisit of an earlier frame (a planted loop closure), 0.5 s per frame"""
    d = np.zeros((n, nbytes), np.uint8)
    cur = rng.integers(0, 256, nbytes, dtype=np.uint8) if base is None else base[-1].copy()
    pool = [] if base is None else list(base)
    for i in range(n):
        if pool and rng.random() < revisit:
            cur = pool[int(rng.integers(0, len(pool)))].copy()
        elif rng.random() < 0.05:
            cur = rng.integers(0, 256, nbytes, dtype=np.uint8)
        for b in rng.integers(0, 8 * nbytes, int(rng.integers(0, 4))):
            cur[b // 8] ^= np.uint8(1 << (b % 8))
        d[i] = cur
        pool.append(cur.copy())
    stamps = t0 + np.arange(n, dtype=np.int64) * (S // 2)
    return d, stamps


def same_knn(g, r):
    pl, di = g.last_knn()
    return np.array_equal(pl, r.last_knn[0]) and np.array_equal(di, r.last_knn[1])


@pytest.mark.parametrize("nbytes,seed,cfg", [(32, 0, dict()), (64, 1, dict()), (32, 2, dict(k_nearest_neighbors=3, T=10.5)),
                                             (64, 3, dict(k_nearest_neighbors=25, T=40.0, min_time_gap=2.0)),
                                             (32, 4, dict(k_nearest_neighbors=0))])
def test_random_sequences_equal_the_reference(capi, nbytes, seed, cfg):
    rng = np.random.default_rng(seed)
    g = capi.Gist(**cfg)
    r = GistReference(**cfg)
    desc, stamps = trajectory(rng, 700, nbytes)
    for i in range(700):
        d = None if rng.random() < 0.08 else desc[i]
        op = rng.random()
        if op < 0.6:
            a, pa = g.search_and_add(d, stamps[i])
            b, pb = r.search_and_add(d, stamps[i])
            assert pa == pb and np.array_equal(a, b), (i, a, b)
            assert same_knn(g, r), i
        elif op < 0.75:
            assert g.add(d, stamps[i]) == r.add(d, stamps[i])
        elif op < 0.9:
            qp = int(rng.integers(-1, r.count() + 3))
            a = g.search(d, stamps[i], query_place=qp)
            b = r.search(d, stamps[i], query_place=qp)
            assert np.array_equal(a, b), (i, a, b)
            assert same_knn(g, r), i
        else:
            live = [p for p in range(r.count()) if r.alive[p]]
            if live:
                p = int(rng.choice(live))
                g.remove(p); r.remove(p)
        assert g.count() == r.count()
    g.close()


def _singles(g, desc, stamps, has=None):
    out = []
    for i in range(len(stamps)):
        d = desc[i] if has is None or has[i] else None
        out.append(g.search_and_add(d, stamps[i]))
    return out


@pytest.mark.parametrize("store", [0, 50000])
def test_batch_equals_single_calls(capi, store):
    rng = np.random.default_rng(10 + store)
    base, bst = trajectory(rng, max(store, 1), 32)
    A, B = capi.Gist(), capi.Gist()
    if store:
        assert A.add_batch(base, bst) == 0 and B.add_batch(base, bst) == 0
    t = int(bst[-1]) + 60 * S
    for n in (1, 255, 256, 257, 2000):
        desc, st = trajectory(rng, n, 32, base=base[-2000:] if store else None, t0=t)
        has = (rng.random(n) > 0.05).astype(np.uint8)
        t = int(st[-1]) + 60 * S
        lists, first, total = A.search_and_add_batch(desc, st, has_gist=has)
        single = _singles(B, desc, st, has)
        assert first == single[0][1] and [p for _, p in single] == list(range(first, first + n))
        for i in range(n):
            assert np.array_equal(lists[i], single[i][0]), (n, i)
        assert total == sum(len(x) for x, _ in single)
        pa, da = A.last_knn(); pb, db = B.last_knn()
        assert np.array_equal(pa, pb) and np.array_equal(da, db)
    assert A.count() == B.count()
    assert total > 0
    A.close(); B.close()


def test_batch_against_the_reference_and_cap_truncation(capi):
    rng = np.random.default_rng(20)
    desc, st = trajectory(rng, 600, 64, revisit=0.3)
    r = GistReference()
    want = [r.search_and_add(desc[i], st[i])[0] for i in range(600)]
    flat = np.concatenate(want)
    assert len(flat) > 50
    g = capi.Gist()
    lists, first, total = g.search_and_add_batch(desc, st)
    assert first == 0 and total == len(flat)
    assert all(np.array_equal(a, b) for a, b in zip(lists, want))
    h = capi.Gist()
    cap = len(flat) // 2
    lists, _, total = h.search_and_add_batch(desc, st, cap=cap)
    assert total == len(flat)
    assert np.array_equal(np.concatenate(lists), flat[:cap])
    g.close(); h.close()


def test_add_batch_equals_add_calls(capi):
    rng = np.random.default_rng(30)
    desc, st = trajectory(rng, 3000, 32)
    has = (rng.random(3000) > 0.1).astype(np.uint8)
    A, B = capi.Gist(), capi.Gist()
    r = GistReference()
    assert A.add_batch(desc, st, has_gist=has) == 0
    for i in range(3000):
        d = desc[i] if has[i] else None
        assert B.add(d, st[i]) == i == r.add(d, st[i])
    assert A.count() == B.count() == 3000
    q, qs = trajectory(rng, 200, 32, base=desc, t0=int(st[-1]) + 100 * S)
    for i in range(200):
        a = A.search_and_add(q[i], qs[i]); b = B.search_and_add(q[i], qs[i]); c = r.search_and_add(q[i], qs[i])
        assert a[1] == b[1] == c[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
        assert same_knn(A, r) and same_knn(B, r)
    # gist-less batches: indices only; an all-gist-less batch before any descriptor is indexed
    E = capi.Gist()
    assert E.add_batch(None, np.zeros(5, np.int64)) == 0 and E.count() == 5
    assert E.search_and_add(desc[0], 100 * S)[1] == 5
    A.close(); B.close(); E.close()


def test_bad_arguments_leave_the_handle_untouched(capi):
    L = capi.lib()
    rng = np.random.default_rng(40)
    desc, st = trajectory(rng, 300, 32, revisit=0.3)
    g = capi.Gist(); r = GistReference()
    for i in range(150):
        assert g.search_and_add(desc[i], st[i])[1] == r.search_and_add(desc[i], st[i])[1]
    # descriptor length differs from the first indexed one
    for call in (lambda: g.search_and_add(np.zeros(64, np.uint8), 0), lambda: g.add(np.zeros(16, np.uint8), 0),
                 lambda: g.search(np.zeros(33, np.uint8), 0), lambda: g.search_and_add_batch(np.zeros((4, 64), np.uint8), np.zeros(4)),
                 lambda: g.add_batch(np.zeros((4, 31), np.uint8), np.zeros(4))):
        with pytest.raises(capi.UzlError) as e:
            call()
        assert e.value.status == capi.UZL_ERR_BAD_ARG
    # unknown place on remove: never given, already removed
    g.remove(3); r.remove(3)
    for p in (3, 150, 10**6, -1):
        with pytest.raises(capi.UzlError) as e:
            g.remove(p)
        assert e.value.status == capi.UZL_ERR_NOT_FOUND
    # NULL outputs
    d = np.ascontiguousarray(desc[150])
    dp = d.ctypes.data_as(capi.c_u8p)
    n = C.c_int32(); idx = C.c_int32(); tot = C.c_int64()
    st1 = np.array([st[150]], np.int64)
    assert L.uzl_gist_search_and_add(g._h, dp, 32, C.c_int64(0), 4, None, C.byref(n), C.byref(idx)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gist_search_and_add(g._h, dp, 32, C.c_int64(0), 0, None, None, C.byref(idx)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gist_search(g._h, dp, 32, C.c_int64(0), -1, 0, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gist_search_and_add_batch(g._h, 1, dp, None, 32, st1.ctypes.data_as(capi.c_i64p), C.c_int64(0), None, None, None,
                                           None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gist_add_batch(g._h, 1, dp, None, 32, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_gist_search_and_add(None, dp, 32, C.c_int64(0), 0, None, C.byref(n), None) == capi.UZL_ERR_BAD_ARG
    assert g.count() == r.count() == 150
    # ... and the handle goes on as if none of it had happened
    for i in range(150, 300):
        a, pa = g.search_and_add(desc[i], st[i]); b, pb = r.search_and_add(desc[i], st[i])
        assert pa == pb and np.array_equal(a, b) and same_knn(g, r)
    g.close()
    for bad in (dict(k_nearest_neighbors=-1), dict(k_nearest_neighbors=257), dict(T=float("nan"))):
        with pytest.raises(capi.UzlError) as e:
            capi.Gist(**bad)
        assert e.value.status == capi.UZL_ERR_BAD_ARG


def test_long_descriptors_and_wide_T(capi):
    """256-byte descriptors, T beyond 8 x bytes (the histogram's last bin), k = 256: everything live is a candidate"""
    rng = np.random.default_rng(50)
    cfg = dict(T=5000.0, k_nearest_neighbors=256, min_time_gap=0.0)
    g = capi.Gist(**cfg); r = GistReference(**cfg)
    d = rng.integers(0, 256, (400, 256), dtype=np.uint8)
    d[::7] = d[0]                                                  # ties
    for i in range(400):
        a, pa = g.search_and_add(d[i], i)
        b, pb = r.search_and_add(d[i], i)
        assert pa == pb and np.array_equal(a, b) and same_knn(g, r), i
    g.close()
