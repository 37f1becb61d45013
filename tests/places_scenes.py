"""Seeded call sequences for the uzl_places_* contract and the call-by-call comparison of its implementations (the restatement
tests/places_reference.py, the CPU checker oracle.Places, the device handle capi.Places).  Shared by test_places_reference.py (CPU)
and test_places_gpu.py."""
import numpy as np

S = 10**9
ALPHABET = np.array([0x00, 0xFF, 0x37, 0xFE], np.uint8)          # for key_width >= 5: keys of random bytes would never collide

# a configuration in which no parameter has its default
CFG = dict(T=2.5, k_nearest_neighbors=3, min_time_gap=2.5, min_rows_to_add=40)


def draw(rng, rows, key_width, nbytes=32, tail_rng=None):
    """rows x nbytes descriptors: the first 32 bytes random (from ALPHABET for key_width >= 5), the bytes from 32 up from tail_rng"""
    head = ALPHABET[rng.integers(0, len(ALPHABET), (rows, 32))] if key_width >= 5 else rng.integers(0, 256, (rows, 32), dtype=np.uint8)
    if nbytes == 32:
        return head
    tail = (tail_rng or rng).integers(0, 256, (rows, nbytes - 32), dtype=np.uint8)
    return np.concatenate([head, tail], axis=1)


def mixed_sequence(seed, key_width, nbytes=32, n_calls=36, rows_lo=64, rows_hi=160, min_rows=CFG["min_rows_to_add"], tail_seed=0):
    """-> list of calls ("search_and_add", desc, stamp) / ("add", desc, stamp) / ("search", desc, stamp, query_place) / ("remove", place, desc).
    Frames share exact copies of rows of a small pool, so every key width finds neighbours; frame sizes include 0, 1, min_rows and
    min_rows + 1; stamps are 1 s apart, so the time gap drops the most recent places; removes name live, dead and unknown ids.
    tail_seed only changes the descriptor bytes from 32 up."""
    rng = np.random.default_rng(seed); tail = np.random.default_rng([seed, tail_seed, 99])
    pool = draw(rng, 300, key_width, nbytes, tail)
    special = {3: 0, 4: 0, 5: 1, 6: 1, 7: min_rows, 8: min_rows, 9: min_rows + 1, 10: min_rows + 1}      # odd: search_and_add, even: add
    ops, kept, n_places = [], {}, 0
    for i in range(n_calls):
        rows = special.get(i, int(rng.integers(rows_lo, rows_hi + 1)))
        d = draw(rng, rows, key_width, nbytes, tail)
        n_copy = int(rng.uniform(0.2, 0.7) * rows)
        if n_copy:
            src = pool[rng.choice(len(pool), n_copy, replace=False)].copy()
            if nbytes > 32:
                src[:, 32:] = tail.integers(0, 256, (n_copy, nbytes - 32), dtype=np.uint8)
            d[:n_copy] = src
        stamp = (1000 + i) * S
        u = rng.random()
        if (i in special and i % 2 == 1) or (i not in special and u < 0.55):
            ops.append(("search_and_add", d, stamp)); kept[n_places] = d; n_places += 1
        elif i in special or u < 0.7:
            ops.append(("add", d, stamp)); kept[n_places] = d; n_places += 1
        else:
            ops.append(("search", d, stamp + 500 * S * int(rng.integers(0, 2)), int(rng.integers(-1, max(n_places, 1)))))
        if i % 6 == 5 and kept:
            k = sorted(kept)[int(rng.integers(0, len(kept)))]
            ops.append(("remove", k, kept.pop(k)))
            if i % 12 == 11:
                ops.append(("remove", k, d))                      # already removed
                ops.append(("remove", n_places + 7, d))           # unknown
    return ops


def apply(impl, op, cap=64):
    """one call on one implementation -> dict(nb, idx, count, counts); counts of the last search / search_and_add"""
    kind = op[0]
    nb, idx = None, None
    if kind == "search_and_add":
        nb, idx = impl.search_and_add(op[1], op[2], cap=cap)
    elif kind == "add":
        idx = impl.add(op[1], op[2])
    elif kind == "search":
        nb = impl.search(op[1], op[2], query_place=op[3], cap=cap)
    elif kind == "remove":
        impl.remove(op[1], op[2])
    else:
        raise ValueError(kind)
    return dict(nb=None if nb is None else [int(x) for x in nb], idx=idx, count=int(impl.count()),
                counts=np.asarray(impl.last_counts(), np.int64))


class OwnSlot:
    """last_counts keeps a search_and_add's own slot (its last one) until the next search: the restatement and the checker hold the
    frame's collisions with itself there, the device 0.  hide() zeroes that slot in the counts read after each call."""

    def __init__(self):
        self.own = None

    def hide(self, kind, counts):
        if kind == "search_and_add":
            self.own = len(counts) - 1
        elif kind == "search" and len(counts):                   # (a search on an empty handle leaves last_counts as they were)
            self.own = None
        c = np.array(counts, np.int64)
        if self.own is not None:
            c[self.own] = 0
        return c


class Runner:
    """Applies calls to every implementation in `impls` (name -> object) and requires, after every call, equal neighbour lists, place
    indices, count() and last_counts.  own_slot: also compare a search_and_add's own slot of last_counts; otherwise it is hidden in
    the comparison and in the results returned."""

    def __init__(self, impls, own_slot=False):
        self.impls, self.own = impls, (None if own_slot else OwnSlot())

    def run(self, ops, cap=64):
        """-> dict(neighbours = number reported in all, calls = per call the first implementation's result)"""
        names = list(self.impls)
        total, calls = 0, []
        for i, op in enumerate(ops):
            res = {n: apply(self.impls[n], op, cap) for n in names}
            if self.own is not None:
                lens = {len(r["counts"]) for r in res.values()}
                assert len(lens) == 1, "call %d (%s): last_counts of %s places" % (i, op[0], sorted(lens))
                for r in res.values():
                    r["counts"] = self.own.hide(op[0], r["counts"])
            a = res[names[0]]
            for n in names[1:]:
                b = res[n]
                where = "call %d (%s): %s vs %s" % (i, op[0], names[0], n)
                assert a["idx"] == b["idx"] and a["count"] == b["count"], where
                assert a["nb"] == b["nb"], "%s: neighbours %s vs %s" % (where, a["nb"], b["nb"])
                ca, cb = a["counts"], b["counts"]
                assert len(ca) == len(cb), where
                assert np.array_equal(ca, cb), "%s: counts differ at places %s" % (where, np.nonzero(ca != cb)[0][:8])
            total += len(a["nb"] or [])
            calls.append(a)
        return dict(neighbours=total, calls=calls)


def run(impls, ops, own_slot=False, cap=64):
    return Runner(impls, own_slot).run(ops, cap)
