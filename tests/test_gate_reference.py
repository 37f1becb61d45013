"""CPU tests (no GPU) of the edge gate's scenes (gate_scenes.py) and its plain-Python reference (gate_reference.py): on every scene
the reference's callback equals the CPU oracle bit by bit, and every scene exercises the case it was built for - asserted here with the
reference alone, so that test_gate_stages_gpu.py never passes on a scene that stopped doing so."""
import functools

import numpy as np
import pytest

import gate_reference as R
import gate_scenes as S


@functools.lru_cache(None)
def traced(name):
    """(accept, valid, dist, trace) of gate_reference.check on a small scene, computed once"""
    sc = S.SMALL[name]()
    tr = []
    a, v, d = R.check(sc["cfg"], sc["poses"], sc["edges"], sc["merged"], sc["cand"], trace=tr)
    return a, v, d, tr


def searches(name):
    return [t for t in traced(name)[3] if t is not None]


@pytest.mark.parametrize("name", sorted(S.SMALL))
def test_reference_equals_oracle(oracle, name):
    sc = S.SMALL[name]()
    o = oracle.Gate(**sc["cfg"]); o.set_graph(sc["poses"], sc["edges"], sc["merged"])
    ao, vo, do = o.check(sc["cand"])
    a, v, d, _ = traced(name)
    assert np.array_equal(a, ao) and np.array_equal(v, vo) and d.tobytes() == do.tobytes()
    assert o.edge_count() == len(sc["edges"]) + int(a.sum())
    o.close()


def test_ties_depend_on_the_id_tie_break(oracle):
    sc = S.ties()
    n = len(sc["poses"])
    assert n == 12 * 12 + 24 and len(sc["pairs"]) == 300
    pos = R.positions(sc["poses"]); adj = R.adjacency(n, sc["edges"])
    o = oracle.Gate(); o.set_graph(sc["poses"], sc["edges"])
    changed = same_place = 0
    for s, t in sc["pairs"].tolist():
        d = R.astar(pos, adj, s, t)[0]
        assert d == o.astar(s, t), (s, t)
        changed += d != R.astar(pos, adj, s, t, reverse_ids=True)[0]
        same_place += s != t and pos[s] == pos[t]
    o.close()
    assert changed >= 5 and same_place >= 1, (changed, same_place)
    # every coordinate is a multiple of 0.25: distances of equal offsets are equal, not nearly equal
    assert np.array_equal(sc["poses"][:, [3, 7, 11]] * 4, np.round(sc["poses"][:, [3, 7, 11]] * 4))


def test_hubs_are_expanded_with_their_twins_open():
    sc = S.hubs()
    n = len(sc["poses"])
    adj = R.adjacency(n, sc["edges"])
    assert tuple(len(adj[h]) for h in sc["hub_ids"]) == S.HUB_DEGREES and 250 <= n <= 350
    tr = searches("hubs")
    for h in sc["hub_ids"]:
        assert sum(1 for t in tr if h in t[1]) >= 3, h
    where = {d: sc["twins"][h][0] for h, d in zip(sc["hub_ids"], S.HUB_DEGREES) if h in sc["twins"]}
    assert where == {9: (3, 7), 65: (63, 64), 129: (70, 100), 200: (10, 140)}
    for h, ((p0, p1), u) in sc["twins"].items():
        assert adj[h][p0] == adj[h][p1] == u and adj[h].count(u) == 2
        hits = [t for t in tr if h in t[1]]
        assert hits and all(u not in t[1][:t[1].index(h)] for t in hits), h      # the twin is not closed when the hub is expanded
    h128 = sc["hub_ids"][S.HUB_DEGREES.index(128)]
    assert adj[h128].count(h128) == 1                                            # the self-loop
    # from the degree-129 hub to its twin: the list ends at exactly gate_reg_kernel<2>'s 128 entries
    h129 = sc["hub_ids"][S.HUB_DEGREES.index(129)]
    k = [q for q in range(len(sc["cand"])) if sc["cand"]["from"][q] == h129 and sc["cand"]["to"][q] == sc["twins"][h129][1]]
    assert len(k) == 1 and traced("hubs")[3][k[0]][2] == 128


def test_components_are_exhausted():
    sc = S.components()
    n = len(sc["poses"])
    adj = R.adjacency(n, sc["edges"])
    seen = {0}; todo = [0]
    while todo:
        for u in adj[todo.pop()]:
            if u not in seen:
                seen.add(u); todo.append(u)
    assert seen == set(range(160))                                               # the largest component, closed under valid non-laser edges
    e = sc["edges"]
    assert any(t == S.LASER and v for t, v in zip(e["type"], e["valid"])) and any(t == S.ODOM and not v for t, v in zip(e["type"], e["valid"]))
    whole = [t for t in searches("components") if t[0] == R.DMAX and len(set(t[1])) >= 150]
    assert len(whole) >= 10 and any(t[3] for t in whole)                         # n_open == 0 with stale entries left in the list
    assert all(set(t[1]) == seen for t in whole)


@pytest.mark.parametrize("name", ["stages", "stages_ssf0", "stages_ssfneg"])
def test_stage_rows_decide_where_they_should(name):
    sc = S.SMALL[name]()
    adj = R.adjacency(len(sc["poses"]), sc["edges"])
    st = {row: R.stage(sc["cfg"], sc["poses"], adj, sc["cand"][k]) for k, row in enumerate(sc["rows"])}
    acc = dict(zip(sc["rows"], traced(name)[0]))
    assert min(s["margin"] for s in st.values()) >= 1e-6                         # gate_decided's 1e-9 and rounding cannot move a row
    got = {row: (s["stage"], s["how"]) for row, s in st.items()}
    if name == "stages":
        assert got == {"i": ("line", "line"), "ii": ("ball", "key"), "iii": ("ball", "exhausted"), "iv": ("search", "target first"),
                       "v": ("search", "target first"), "vi": ("line", "line"), "vii": ("ball", "key"), "viii": ("line", "line"),
                       "xi": ("search", "target first")}
        assert [int(acc[r]) for r in sc["rows"]] == [1, 1, 1, 1, 0, 1, 1, 1, 0]
        d = dict(zip(sc["rows"], traced(name)[2]))
        assert d["iii"] == R.DMAX and d["viii"] == 0.0 and abs(d["iv"] - 6.3667) < 1e-3
    elif name == "stages_ssf0":
        assert {s for s, _ in got.values()} == {"line", "ball", "search"}        # the tests no longer depend on the path length
        assert [int(acc[r]) for r in sc["rows"]] == [1, 0, 1, 0, 0, 1, 0, 1, 0]
    else:
        assert set(got.values()) == {("search", "not monotone")}
        assert 0 < sum(int(a) for a in acc.values()) < len(acc)


def test_escalation_has_every_list_class():
    sc = S.escalation()
    peaks = np.array([t[2] for t in searches("escalation")])
    assert 100 <= len(sc["poses"]) <= 999 and len(sc["cand"]) <= 256             # one launch chunk: no class hides behind another's escalation
    assert (peaks <= 128).sum() >= 2 and ((peaks > 128) & (peaks <= 256)).sum() >= 2 and (peaks > 256).sum() >= 2


def test_chunks_cross_the_chunk_edge():
    sc = S.chunks()
    a, v, d, _ = traced("chunks")
    c = sc["cand"]
    assert len(c) >= 600 and len(sc["poses"]) <= 100
    assert v[:256].sum() >= 1 and v[256:512].sum() >= 1
    assert (c["from"][255], c["to"][255], c["type"][255]) == (c["to"][256], c["from"][256], c["type"][256])
    assert a[255] == 1 and v[255] == 1 and a[256] == 0 and d[256] == -1.0          # refused by existsEdge, across the chunk edge


@pytest.mark.parametrize("n", S.BITMAP_SIZES)
def test_bitmap_edges_end_at_the_last_node(n):
    sc = S.bitmap_edges(n)
    c = sc["cand"]
    assert len(sc["poses"]) == n and ((c["from"] == n - 1) | (c["to"] == n - 1)).sum() >= 2
    if n > 1024:
        adj = R.adjacency(n, sc["edges"])
        ids = sorted(set(adj[0]) | {0})
        diffs = {abs(a - b) for a in ids for b in ids}
        assert 1024 in adj[0] and 1024 in diffs and (n < 2081 or (2048 in adj[0] and {7, 7 + 1024, 7 + 2048} <= set(ids))) and len(adj[0]) <= 64
        assert any(0 in t[1] for t in searches("bitmap_edges_%d" % n))            # and a search expands that node


@pytest.mark.parametrize("n", [S.LARGE_LAST_LDS, S.LARGE_FIRST_WAVE])
def test_large_sizes_and_the_overflowing_search(n):
    """n and the open-list condition only (the oracle checks these scenes in test_gate_stages_gpu.py)"""
    sc = S.large(n)
    assert len(sc["poses"]) == n and len(sc["cand"]) <= 8
    lds = lambda m: 32 * 32 * 64 + 32 * 4 + 2 * 4 * ((m + 31) // 32)              # gate_lds_bytes of gate_types.hpp
    assert (lds(n) == 160 * 1024 - 2048) if n == S.LARGE_LAST_LDS else (lds(n) > 160 * 1024 - 2048 >= lds(n - 1))
    adj = R.CsrAdjacency(n, sc["edges"])
    pos = sc["poses"][:, [3, 7, 11]]
    c = sc["cand"]; rows = list(sc["rows"])
    k = rows.index("cluster")
    assert R.astar(pos, adj, int(c["from"][k]), int(c["to"][k]))[2] > 2048        # kGateOpenCap
    H = sc["hub"]
    assert len(adj[H]) == 130 and adj[H][63] == adj[H][64]
    k = rows.index("hub")
    d, expanded, peak, _ = R.astar(pos, adj, int(c["from"][k]), int(c["to"][k]))
    assert H in expanded and adj[H][63] not in expanded[:expanded.index(H)] and d < R.DMAX
    assert c["to"][rows.index("last node")] == n - 1 and c["from"][rows.index("last word")] == n - 1
    assert abs(int(c["to"][rows.index("long walk")]) - int(c["from"][rows.index("long walk")])) <= 20000
