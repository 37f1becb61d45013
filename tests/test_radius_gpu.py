"""uzl_radius_* on the device: bit-exact against the CPU checker (element for element, in order) and equal to the NumPy restatement
(tests/radius_reference.py) outside the threshold band, at the node counts around the 64-lane wave and the 256-node slab, with dense
and sparse hit patterns that have known answers, rotations up to 180 degrees, thresholds that are met exactly, epoch-sized stamps,
odd query lists, output caps and replaced node sets."""
import ctypes as C

import numpy as np
import pytest

import radius_reference as RR
import radius_scenes as RS

pytestmark = pytest.mark.gpu
S = RS.S


def both(capi, oracle, P, st, q, cfg, band=RS.BAND, handle=None):
    """query on the device and the checker; exact equality; the restatement outside the band -> (jobs, counts)"""
    q = np.asarray(q, np.int32)
    full = dict(radius=0.5, new_edge_time=5.0, max_rotation_deg=30.0); full.update(cfg)
    f, t, cnt = oracle.radius_candidates(P, st, q, **full)
    r = handle or capi.Radius(**cfg)
    if handle is None:
        r.set_nodes(P, st)
    gf, gt, gcnt, tot = r.query(q)
    if handle is None:
        r.close()
    assert tot == len(f) and np.array_equal(gf, f) and np.array_equal(gt, t) and np.array_equal(gcnt, cnt)
    jobs = list(zip(gf.tolist(), gt.tolist()))
    RS.check_against_restatement(jobs, P, st, q, full, band=band)
    return jobs, gcnt


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1025])
def test_node_counts_at_wave_and_slab_edges(capi, oracle, n):
    P, st = RS.cloud(n, seed=1000 + n)
    jobs, _ = both(capi, oracle, P, st, np.arange(n), dict(radius=1.0, max_rotation_deg=170.0))
    assert len(jobs) > n or n <= 2


@pytest.mark.parametrize("n", [2, 64, 65, 256, 257, 1025])
def test_dense_append(capi, oracle, n):
    """every node within the radius of every other, identity rotations, stamps far apart: the jobs of query q are 0 .. n-1 without q,
    ascending - full ballots, a hit in lane 63, every wave and slab seam"""
    rng = np.random.default_rng(n)
    P = RS.identity_nodes(rng.uniform(0, 0.1, (n, 3))); st = (10 * S * np.arange(n)).astype(np.int64)
    q = np.unique(np.r_[0, 1, 62, 63, 64, 255, 256, n // 2, n - 2, n - 1].clip(0, n - 1))
    jobs, cnt = both(capi, oracle, P, st, q, dict(radius=0.5))
    assert jobs == [(c, int(qq)) for qq in q for c in range(n) if c != qq] and list(cnt) == [n - 1] * len(q)


@pytest.mark.parametrize("pattern", ["last_partial_slab", "lanes_0_and_63", "lane_63_only", "one_per_slab"])
def test_sparse_hit_patterns(capi, oracle, pattern):
    n = 1025 if pattern != "last_partial_slab" else 600
    c = np.arange(n)
    near = {"last_partial_slab": c >= 512, "lanes_0_and_63": (c % 64 == 0) | (c % 64 == 63), "lane_63_only": c % 64 == 63,
            "one_per_slab": c % 256 == 129}[pattern]
    rng = np.random.default_rng(5)
    t = rng.uniform(0, 0.1, (n, 3)); t[~near] += 100. + rng.uniform(0, 1000., ((~near).sum(), 3))       # the others: far from all
    near[7] = True; t[7] = 0.05                                                  # a query node in the first slab, inside the cluster
    P = RS.identity_nodes(t); st = (10 * S * c).astype(np.int64)
    hits = np.nonzero(near)[0]
    q = [7, int(hits[-1]), 8]
    jobs, cnt = both(capi, oracle, P, st, q, dict(radius=0.5))
    assert jobs == [(int(h), 7) for h in hits if h != 7] + [(int(h), int(hits[-1])) for h in hits[:-1]] and list(cnt) == [len(hits) - 1] * 2 + [0]


@pytest.mark.parametrize("max_rot", [100., 170., 181.])
def test_large_rotations(capi, oracle, max_rot):
    """relative rotations up to 180 degrees: the trace <= 0 branch of the quaternion conversion decides (angle = 360 - theta for w < 0)"""
    P, st = RS.cloud(513, seed=31)
    cfg = dict(radius=1.0, new_edge_time=5.0, max_rotation_deg=max_rot)
    jobs, _ = both(capi, oracle, P, st, np.arange(513), cfg)
    plain = RR.candidates(P, st, np.arange(513), plain_angle=True, **cfg)[0]
    assert len(jobs) > 500
    if max_rot == 100.:
        assert jobs == plain                                      # the branch runs from 120 degrees on: both readings are above 100
    else:
        assert set(jobs) < set(plain) and len(plain) - len(jobs) > 50


def test_thresholds_met_exactly(capi, oracle):
    """0.25 m steps, 2 s stamps: a distance equal to the radius and a gap equal to new_edge_time are not hits (no band here)"""
    n = 40
    P = RS.identity_nodes(np.stack([0.25 * np.arange(n), np.zeros(n), np.zeros(n)], axis=1)); st = (2 * S * np.arange(n)).astype(np.int64)
    for cfg, reach in ((dict(radius=0.75, new_edge_time=3.0), [2]), (dict(radius=1.0, new_edge_time=4.0), [3]),
                       (dict(radius=1.0, new_edge_time=6.0), []), (dict(radius=2.5, new_edge_time=8.0), [5, 6, 7, 8, 9])):
        jobs, _ = both(capi, oracle, P, st, [20, 0], cfg, band=0.0)
        assert jobs == [(20 + s * k, 20) for s in (-1, 1) for k in (reach[::-1] if s < 0 else reach)] + [(k, 0) for k in reach], cfg


def test_epoch_sized_stamps(capi, oracle):
    """stamps of about 1.7e18 ns with gaps of new_edge_time +- 1 us (and +- 1 ns): the difference is taken on the integers"""
    base = 1_700_000_000 * S + 987_654_321
    for eps in (1000, 1):
        gaps = np.array([0, 5 * S - eps, 5 * S, 5 * S + eps, 10 * S + eps, 10 * S + 2 * eps, 15 * S + 2 * eps], np.int64)
        P = RS.identity_nodes(np.zeros((len(gaps), 3))); st = base + gaps
        jobs, _ = both(capi, oracle, P, st, [0, 3, 4], dict(radius=0.5, new_edge_time=5.0), band=0.0)
        # from node 0: gaps as listed.  From node 3 (5 s + eps): node 4 is exactly 5 s away, node 5 5 s + eps.  From node 4: node 1 is
        # 5 s + 2 eps away, node 2 5 s + eps, node 3 exactly 5 s, node 6 5 s + eps
        assert jobs == [(3, 0), (4, 0), (5, 0), (6, 0), (0, 3), (5, 3), (6, 3), (0, 4), (1, 4), (2, 4), (6, 4)], eps


def test_query_lists(capi, oracle):
    P, st = RS.cloud(300, seed=41)
    cfg = dict(radius=1.0, max_rotation_deg=360.0)
    r = capi.Radius(**cfg); r.set_nodes(P, st)
    one, cnt1 = both(capi, oracle, P, st, [17], cfg, handle=r)
    assert len(one) == cnt1[0] > 5
    dup, cnt = both(capi, oracle, P, st, [17, 17, 5, 17], cfg, handle=r)
    assert dup[:len(one)] == one == dup[len(one):2 * len(one)] == dup[-len(one):] and list(cnt[[0, 1, 3]]) == [len(one)] * 3
    bad, cnt = both(capi, oracle, P, st, [-1, 300, 2**31 - 1, -2**31], cfg, handle=r)
    assert bad == [] and list(cnt) == [0, 0, 0, 0]
    mixed, cnt = both(capi, oracle, P, st, [300, 17, -1], cfg, handle=r)
    assert mixed == one and list(cnt) == [0, len(one), 0]
    assert r.query(np.zeros(0, np.int32))[3] == 0
    r.close()


def test_cap_truncation(capi, oracle):
    """cap in the middle of a query's block, exactly at a block boundary, and 0: the total and the per-query counts stay full, the
    prefix is written and nothing after it"""
    P, st = RS.cloud(400, seed=51)
    q = np.array([3, 250, 77, 399], np.int32)
    f, t, cnt = oracle.radius_candidates(P, st, q, radius=1.0, max_rotation_deg=360.0)
    assert cnt.min() >= 4
    r = capi.Radius(radius=1.0, max_rotation_deg=360.0); r.set_nodes(P, st)
    ends = np.cumsum(cnt)
    for cap in (0, 1, int(ends[0]) - 1, int(ends[0]), int(ends[0]) + 1, int(ends[1]), int(ends[2]) + 2, int(ends[3]) - 1, int(ends[3]), int(ends[3]) + 5):
        gf, gt, gcnt, tot = r.query(q, cap=cap)
        w = min(cap, len(f))
        assert tot == len(f) and np.array_equal(gcnt, cnt) and np.array_equal(gf, f[:w]) and np.array_equal(gt, t[:w]), cap
    # the caller's buffers beyond cap stay untouched
    bf = np.full(len(f) + 8, -7, np.int32); bt = np.full(len(f) + 8, -7, np.int32); tot = C.c_int64()
    cap = int(ends[1]) + 1
    rc = capi.lib().uzl_radius_query(r._h, C.c_int32(4), q.ctypes.data_as(capi.c_i32p), C.c_int64(cap), bf.ctypes.data_as(capi.c_i32p),
                                     bt.ctypes.data_as(capi.c_i32p), None, C.byref(tot))
    assert rc == capi.UZL_OK and tot.value == len(f) and np.array_equal(bf[:cap], f[:cap]) and (bf[cap:] == -7).all() and (bt[cap:] == -7).all()
    r.close()


def test_set_nodes_replacement(capi, oracle):
    """set_nodes again with fewer and then more nodes: queries see exactly the current set - no stale node, no stale pose"""
    cfg = dict(radius=1.0, max_rotation_deg=360.0)
    r = capi.Radius(**cfg)
    for n, seed in ((700, 1), (90, 2), (0, 3), (1300, 4), (1, 5), (257, 6)):
        P, st = RS.cloud(n, seed=60 + seed)
        r.set_nodes(P, st)
        q = np.r_[np.arange(0, max(n, 1), max(n // 40, 1)), [n, 89, 699, 1299, 0]]
        jobs, cnt = both(capi, oracle, P, st, q, cfg, handle=r)
        assert all(c < n and t < n for c, t in jobs) and (len(jobs) > 50 or n <= 1)
    r.close()
