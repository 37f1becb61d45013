"""Seeded node sequences for the uzl_gfr_* tests and tests/diag/gfr_timing.py, and their replay through tests/gfr_reference.py.

A world of landmark descriptors; a node sees a location (a set of landmarks), each landmark with 0-12 bits flipped; locations are
revisited; about 8 % of the nodes carry no features.  Planted into every sequence: beacons queried at distance exactly
max_distance - 1 and max_distance, rows with exactly 3 * bytes and 3 * bytes + 1 set bits, exact duplicate features that a later
row ties on, and nodes that see one landmark twice (a duplicate link)."""
import functools

import numpy as np

from gfr_reference import GfrReference

S = 10**9

CONFIGS = {
    "defaults": dict(),
    "T10.5-k3": dict(T=10.5, k_nearest_neighbors=3),
    "k0": dict(k_nearest_neighbors=0),
    "d25-gap2": dict(max_distance=25, min_time_gap=2.0),
}


def flip(rng, row, nbits):
    """row with exactly nbits distinct bits flipped"""
    out = row.copy()
    for b in rng.choice(8 * len(row), int(nbits), replace=False):
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def sparse_row(rng, nbytes, bits):
    """a row with exactly `bits` set bits"""
    return flip(rng, np.zeros(nbytes, np.uint8), bits)


def dense_rows(rng, n, nbytes):
    """random rows that pass the popcount rule (popcount > 3 * bytes)"""
    d = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
    while True:
        bad = np.flatnonzero(np.bitwise_count(d).sum(axis=1) <= 3 * nbytes)
        if not len(bad):
            return d
        d[bad] = rng.integers(0, 256, (len(bad), nbytes), dtype=np.uint8)


def nodes(seed, nbytes, max_distance=40, n_nodes=300, n_landmarks=1500):
    """[(op, desc or None, stamp_ns, query_place draw in [0, 1))]: op in "search_and_add", "add", "search", "remove" """
    rng = np.random.default_rng(seed)
    land = dense_rows(rng, n_landmarks, nbytes)
    beacons = dense_rows(rng, 4, nbytes)                   # [3]: stored twice by one node, never on its own
    # where the plants go: beacons stored early by a call that integrates, queried later by a call that matches
    plant = {4: ("store", None), 40: ("near", 0), 60: ("far", 1), 41: ("dup", None), 80: ("dup_query", None)}
    locations, out = [], []
    for i in range(n_nodes):
        u = rng.random()
        op = "search_and_add" if u < 0.6 else "add" if u < 0.75 else "search" if u < 0.9 else "remove"
        old = [j for j in range(len(locations)) if j <= i - 15 and locations[j] is not None]
        if old and rng.random() < 0.4:
            loc = locations[int(rng.choice(old))]
            loc = loc[rng.random(len(loc)) < 0.9] if len(loc) > 25 else loc
        else:
            loc = rng.choice(n_landmarks, int(rng.integers(20, 91)), replace=False)
        rows = [flip(rng, land[l], rng.integers(0, 13)) for l in loc]
        if rng.random() < 0.15:                                    # one landmark seen twice
            rows.append(flip(rng, land[loc[0]], rng.integers(0, 13)))
        if rng.random() < 0.2:                                     # the popcount rule's two sides
            rows.append(sparse_row(rng, nbytes, 3 * nbytes))
            rows.append(sparse_row(rng, nbytes, 3 * nbytes + 1))
        featureless = rng.random() < 0.08
        what = plant.get(i)
        if what:
            op, featureless = "search_and_add", False
            if what[0] == "store":
                rows.extend(beacons[:3])
            elif what[0] == "near":
                rows.append(flip(rng, beacons[what[1]], max_distance - 1))
            elif what[0] == "far":
                rows.append(flip(rng, beacons[what[1]], max_distance))
            elif what[0] == "dup":
                rows.extend([beacons[3], beacons[3]])                # both unmatched: two identical features
            else:
                rows.append(flip(rng, beacons[3], 3))                # a tie at distance 3: the lower index
        locations.append(None if featureless or op in ("search", "remove") else np.asarray(loc))
        desc = None if featureless else np.stack(rows)
        out.append((op, desc, i * (S // 2), rng.random()))
    return out


def replay_reference(seq, cfg, feature_type=2):
    """the sequence through GfrReference: per step what a handle must give, then the final repository"""
    r = GfrReference(**cfg)
    steps = []
    for op, desc, stamp, draw in seq:
        st = dict(op=op, desc=desc, stamp=stamp)
        if op == "search_and_add":
            st["neighbours"], st["place"] = r.search_and_add(desc, stamp, feature_type)
        elif op == "add":
            st["place"] = r.add(desc, stamp, feature_type)
        elif op == "search":
            st["query_place"] = int(draw * (r.count() + 3)) - 1
            st["neighbours"] = r.search(desc, stamp, feature_type, st["query_place"])
        else:
            live = [p for p in range(r.count()) if r.alive[p]]
            st["remove"] = live[int(draw * len(live))] if live else None
            if live:
                r.remove(st["remove"])
        st.update(matches=(r.last_matches[0].copy(), r.last_matches[1].copy()), votes=r.last_votes.copy(), count=r.count(),
                  F=r.feature_count(), L=r.link_count())
        steps.append(st)
    features = [r.get_feature(f) for f in range(r.F)]
    return steps, features, dict(r.counters), r


@functools.lru_cache(maxsize=None)
def trace(nbytes, cfg_name, seed, n_nodes=300):
    """computed once per process, shared by the tests that replay it; nobody changes it"""
    cfg = CONFIGS[cfg_name]
    return replay_reference(nodes(seed, nbytes, cfg.get("max_distance", 40), n_nodes), cfg)[:3]


def replay_handle(g, steps, nbytes, feature_type=2, check=None):
    """the steps through a capi.Gfr; returns per step everything the handle gave (check(i, got, step) is called after each)"""
    outs = []
    for i, st in enumerate(steps):
        got = dict()
        if st["op"] == "search_and_add":
            got["neighbours"], got["place"] = g.search_and_add(st["desc"], st["stamp"], feature_type)
        elif st["op"] == "add":
            got["place"] = g.add(st["desc"], st["stamp"], feature_type)
        elif st["op"] == "search":
            got["neighbours"] = g.search(st["desc"], st["stamp"], feature_type, st["query_place"])
        elif st["remove"] is not None:
            g.remove(st["remove"])
        got.update(matches=g.last_matches(), votes=g.last_votes(), count=g.count(), F=g.feature_count(), L=g.link_count())
        if check:
            check(i, got, st)
        outs.append(got)
    return outs


def same_step(i, got, st):
    for key in ("place", "count", "F", "L"):
        if key in st:
            assert got[key] == st[key], (i, st["op"], key, got[key], st[key])
    if "neighbours" in st:
        assert np.array_equal(got["neighbours"], st["neighbours"]), (i, st["op"], got["neighbours"], st["neighbours"])
    assert np.array_equal(got["matches"][0], st["matches"][0]), (i, st["op"], "matched features")
    assert np.array_equal(got["matches"][1], st["matches"][1]), (i, st["op"], "nearest distances")
    assert np.array_equal(got["votes"], st["votes"]), (i, st["op"], "votes")


def same_features(g, features, nbytes):
    assert g.feature_count() == len(features)
    for f, (desc, places) in enumerate(features):
        d, pl = g.get_feature(f, nbytes)
        assert np.array_equal(d, desc) and np.array_equal(pl, places), f
