"""CPU tests of tests/width_scenes.py: under the references alone, every scene of test_descriptor_widths_gpu.py holds what it
claims - the planted ties, cuts, boundaries and paddings are there - so that a pass on the device cannot be an empty one."""
import numpy as np
import pytest

import gfr_scenes as G
import width_scenes as WS
from gfr_reference import GfrReference
from gist_reference import brute_knn, hamming
from oracle import wire as OW
from test_wire import _frame, _node
from uzliti_slam_amd import wire as W


# ------------------------------------------------------------------------------------------------ matcher
@pytest.mark.parametrize("nbytes", WS.KNN2_WIDTHS)
def test_knn2_scenes_hold_their_ties(oracle, nbytes):
    assert nbytes % 4 == 0 and nbytes // 4 not in (8, 16)                    # none of these takes a fast path
    for nq, nt in WS.KNN2_SHAPES:
        q, t = WS.knn2_case(nq, nt, nbytes)
        assert q.shape == (nq, nbytes) and t.shape == (nt, nbytes)
        i0, d0, i1, d1 = oracle.knn2(q, t)
        assert (i0 >= 0).all() and (i1 >= 0).all() and (d0 <= d1).all()
        if nt >= 8:
            # four copies of t[2] (rows 2, 5, 7, nt - 1): the two lowest win, at distance 0 and, one bit off, 1
            assert (i0[0], d0[0], i1[0], d1[0]) == (2, 0, 5, 0)
            assert (i0[1], d0[1], i1[1], d1[1]) == (2, 1, 5, 1)
        if nq >= 8 and nt >= 8:
            assert (i0[2], d0[2]) == (4, 0) and (i0[3], d0[3]) == (3, 0) and (i0[4], d0[4]) == (4, 0) and (i0[5], d0[5]) == (3, 1)
        for row in range(0, nq, max(1, nq // 5)):                            # the oracle against plain popcounts
            d = hamming(q[row], t)
            order = np.lexsort((np.arange(nt), d))
            assert (i0[row], d0[row], i1[row], d1[row]) == (order[0], d[order[0]], order[1], d[order[1]])


def test_knn2_largest_distance_at_508_bytes(oracle):
    (q1, t1), (q2, t2), (q3, t3) = WS.knn2_extreme_case(508)
    i0, d0, i1, d1 = oracle.knn2(q1, t1)
    assert (i0[0], d0[0], i1[0], d1[0]) == (0, 4064, -1, -1)
    i0, d0, i1, d1 = oracle.knn2(q2, t2)
    assert (i0[0], d0[0], i1[0], d1[0]) == (1, 0, 0, 4064) and (i0[1], d0[1], i1[1], d1[1]) == (0, 0, 1, 4064)
    i0, d0, i1, d1 = oracle.knn2(q3, t3)
    assert (i0[0], d0[0], i1[0], d1[0]) == (0, 4064, 1, 4064) and (i0[1], d0[1], i1[1], d1[1]) == (0, 0, 1, 0)
    assert 4064 < 2**12                                                       # what the packed key leaves above 20 index bits


@pytest.mark.parametrize("nbytes", WS.EST_WIDTHS + (32, 64))
def test_estimate_scenes_have_a_consensus(oracle, nbytes):
    for j, (f, t, T) in enumerate(WS.est_pairs(nbytes)):
        assert f["desc"].shape == t["desc"].shape == (WS.EST_KP, nbytes)
        w = WS.oracle_edge(oracle, [f], [t], j)
        assert w["ok"] == 1 and w["consensus"] > 50, (nbytes, j, w["consensus"])
        assert np.abs(w["T"] - T).max() < 0.05                              # ... and it is the motion the frames were made with


def test_mixed_batch_is_what_it_claims(oracle):
    jobs = WS.mixed_batch()
    assert len(jobs) == 10 and len({jid for _, _, jid in jobs}) == 10
    assert [fr[0]["desc"].shape[1] for fr, _, _ in jobs[:8]] == [32, 64, 20, 48] * 2
    assert sorted(sum(WS.mixed_batch_groups(), [])) == list(range(10))
    for g, nb in zip(WS.mixed_batch_groups()[:4], WS.MIXED_WIDTHS):
        assert all(jobs[j][0][0]["desc"].shape[1] == jobs[j][1][0]["desc"].shape[1] == nb for j in g)
    want = [WS.oracle_edge(oracle, fr, to, jid) for fr, to, jid in jobs]
    assert all(w["ok"] == 1 and w["consensus"] > 50 for w in want[:9])
    # two FeatureData per node: of the four combos only (0, 1) (32 bytes) and (1, 0) (20 bytes) have one width
    fr, to, jid = jobs[8]
    assert [x["desc"].shape[1] for x in fr] == [32, 20] and [x["desc"].shape[1] for x in to] == [20, 32]
    both = [WS.oracle_edge(oracle, [fr[a]], [to[b]], jid) for a, b in ((0, 1), (1, 0))]
    assert all(w["ok"] == 1 for w in both)
    best = 0 if both[0]["n_matches"] >= both[1]["n_matches"] else 1           # more ratio-test survivors; the first wins ties
    assert (want[8]["frame_from"], want[8]["frame_to"]) == ((0, 1), (1, 0))[best]
    assert want[8]["n_matches"] == both[best]["n_matches"] and np.array_equal(want[8]["T"], both[best]["T"])
    # 32 bytes against 64: nothing to pair
    assert want[9]["ok"] == 0 and want[9]["frame_from"] == -1 and want[9]["n_corr"] == 0


# ------------------------------------------------------------------------------------------------ global feature repository
@pytest.mark.parametrize("nbytes,cfg_name,seed", WS.GFR_CASES, ids=[f"{b}-{n}" for b, n, _ in WS.GFR_CASES])
def test_gfr_sequences_show_the_planted_cases(nbytes, cfg_name, seed):
    assert (nbytes + 15) // 16 in (1, 3)
    steps, features, counters = G.trace(nbytes, cfg_name, seed)
    assert counters["neighbours"] >= 50 and counters["vote_ties"] >= 1 and counters["duplicate_links"] >= 1, counters
    assert counters["popcount_drops"] >= 1 and counters["at_max_minus_1"] >= 1 and counters["at_max"] >= 1, counters
    assert len(features) > 500 and all(len(d) == nbytes for d, _ in features[:5])


@pytest.mark.parametrize("nbytes", sorted(WS.GFR_BOUNDARY))
def test_gfr_boundary_scene(nbytes):
    cfg = WS.GFR_BOUNDARY[nbytes]
    planted = WS.gfr_planted(nbytes)
    F = WS.GFR_BOUNDARY_F[-1]
    r = GfrReference(**cfg)
    for f0 in range(0, F, 4096):
        r.add(planted[f0:min(F, f0 + 4096)], 0)
    assert r.feature_count() == F                                            # every row became a feature of its own
    for Fs in WS.GFR_BOUNDARY_F:
        t = WS.gfr_targets(Fs)
        assert {0, Fs - 1} <= set(t) and all(x in t for x in (511, 512, 1023, 1024, 4095, 4096) if x < Fs)
    picks = set()
    for pick, q, keep in WS.gfr_boundary_queries(nbytes, F):
        r.search(q, 100 * WS.S)
        ft, di = r.last_matches
        assert np.array_equal(ft[keep], pick[keep]) and (di[keep] <= 5).all() and (ft[~keep] == -1).all()
        picks.update(pick[keep].tolist())
        for row in (0, len(q) - 1):                                          # the u64 search against byte-table popcounts
            d = hamming(q[row], planted[:F])
            assert d.min() == di[row] and (not keep[row] or d.argmin() == ft[row])
    assert {0, 511, 512, 1023, 1024, 4095, 4096} <= picks                    # both sides of the tile bounds are asked for


# ------------------------------------------------------------------------------------------------ binary GIST
@pytest.mark.parametrize("nbytes", WS.GIST_WIDTHS)
def test_gist_sequences(nbytes):
    for name in ("defaults", "clamp"):
        steps = WS.gist_trace(nbytes, name)
        searched = [st for st in steps if "knn" in st and st["desc"] is not None]
        assert len(searched) > 150 and sum(len(st["knn"][0]) > 0 for st in searched) > 100
        assert sum(len(st["neighbours"]) for st in searched) > 20
        assert any(st["op"] == "remove" and st["remove"] is not None for st in steps)
        if name == "clamp":                                                  # T >= bits: every live place is a candidate, k = 25 cuts
            assert all(len(st["knn"][0]) == min(25, st["candidates"]) for st in searched)
            assert any(st["candidates"] > 25 for st in searched)


@pytest.mark.parametrize("nbytes", WS.GIST_WIDTHS)
def test_gist_quota_scene(nbytes):
    desc, stamps, query = WS.gist_quota_scene(nbytes)
    far = 6 if nbytes > 1 else 4
    d = hamming(query, desc)
    planted = np.array(WS.GIST_QUOTA_PLANTED)
    assert (d[planted] == 3).all() and (np.delete(d, planted) == far).all()
    adds, (nb1, knn1), (nb2, knn2) = WS.gist_quota_trace(nbytes)
    assert [p for _, p, _ in adds] == list(range(WS.GIST_QUOTA_N))
    # eleven places at the cutoff distance, ten slots: the ten lowest indices, 512 is cut
    assert knn1[0].tolist() == [62, 63, 64, 65, 254, 255, 256, 257, 510, 511] and (knn1[1] == 3).all()
    assert nb1.tolist() == knn1[0].tolist()
    # four of them gone: the seven left, then the three lowest places at the next distance
    assert knn2[0].tolist() == [62, 65, 254, 257, 510, 511, 512, 0, 1, 2] and knn2[1].tolist() == [3] * 7 + [far] * 3
    assert nb2.tolist() == knn2[0].tolist()
    alive = [True] * WS.GIST_QUOTA_N
    assert brute_knn(list(desc), alive, query, 10, 10.0) == list(zip(knn1[0].tolist(), knn1[1].tolist()))
    # while the places go in, every planted place after the first finds the earlier ones at distance 0, the others tie at 3 and 6
    assert adds[512][2][0].tolist() == list(WS.GIST_QUOTA_PLANTED[:10]) and (adds[512][2][1] == 0).all()
    if nbytes > 1:
        assert query[-1] != desc[62][-1]                                     # the row's last bit differs: next to the padding


# ------------------------------------------------------------------------------------------------ wire records
@pytest.mark.parametrize("D", WS.WIRE_WIDTHS)
def test_wire_node_scene(D):
    kpb = WS.wire_kpb(D)
    stride = 41 + 4 * D
    assert kpb * stride <= 16368 and (kpb == 128 or (kpb + 1) * stride > 16368)
    counts = WS.wire_counts(D)
    assert counts[5] == 0 and 0 not in counts[:5] + counts[6:] and max(counts) > 2 * kpb
    rng = np.random.default_rng(4000 + D)
    frames = [_frame(rng, n, D) for n in counts]
    node = _node(rng, 1, frames)
    b = OW.encode_node(node)
    assert W.encode_node(node) == b
    sens = W.decode_node(b).fields["sensors"]
    for s, (desc, pos, valid, uv), n in zip(sens, frames, counts):
        assert s["n_features"] == n and s["desc_len"] == (D if n else 0) and len(s["records"]) == n * stride
        if n:
            assert s["uniform"] == 1 and s["records"] == OW.features_pack(desc, pos, valid, uv)
            d, p, v, u = OW.features_unpack(s["records"], n, D)
            assert np.array_equal(d, desc) and np.array_equal(p.view(np.uint64), pos.view(np.uint64))
            assert np.array_equal(v, valid) and np.array_equal(u, uv)
    big = frames[-1]
    assert 0 < big[2].sum() < len(big[2])                                    # valid and invalid keypoints
