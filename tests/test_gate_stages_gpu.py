"""The edge acceptance gate (uzl_gate_*) stage by stage on the scenes of gate_scenes.py: the straight-line shortcut, gate_bound_kernel,
gate_reg_kernel<2> / <4>, gate_wave_kernel, gate_kernel and the host's replay over chunks of 256 candidates.  Verdicts identical to the
CPU oracle and search distances bit-identical, candidate by candidate; which launch wrote a candidate's outputs is read back through
uzl_debug_gate_stages (the diagnostic library) and compared with what gate_reference predicts from the search's largest open list.
test_gate_reference.py asserts, without a GPU, that every scene exercises its case."""
import numpy as np
import pytest

import gate_reference as R
import gate_scenes as S
from test_gate_reference import traced

pytestmark = pytest.mark.gpu

SINGLE_PASS = ["hubs", "ties", "components"] + ["bitmap_edges_%d" % n for n in S.BITMAP_SIZES]    # no valid accept, no escalation before a later chunk
_expected = {}


def expected(oracle, key, sc):
    """the oracle's (accept, valid, dist, edge_count, accept of a second call) on a scene, computed once"""
    if key not in _expected:
        o = oracle.Gate(**sc["cfg"]); o.set_graph(sc["poses"], sc["edges"], sc["merged"])
        a, v, d = o.check(sc["cand"])
        ne = o.edge_count()
        a2, _, _ = o.check(sc["cand"])
        o.close()
        _expected[key] = (a, v, d, ne, a2)
    return _expected[key]


def same(got, exp):
    a, v, d = got
    return np.array_equal(a, exp[0]) and np.array_equal(v, exp[1]) and (d is None or d.tobytes() == exp[2].tobytes())


def code_of(peak):
    """the launch that ends a search on a fresh handle in a single pass, from the search's largest open list: gate_reg_kernel<2> holds
    128 entries, <4> 256; what outgrows both goes to gate_kernel"""
    return 2 if peak <= 128 else 3 if peak <= 256 else 5


def predicted(name):
    """Stage codes of a scene without valid accepts (the adjacency never changes) on a fresh handle with want_dist=True, from the
    reference alone.  The host refuses (0) what is out of range, merged or in the graph when the candidate's chunk of 256 starts; a
    duplicate of a candidate accepted in the same chunk is searched all the same and dropped in the replay.  Every other candidate is
    written by gate_reg_kernel: <2> (2) until a search of an earlier chunk has outgrown 128 entries, <4> (3) from then on and for a
    search of this chunk that outgrows them, gate_kernel (5) beyond 256."""
    sc = S.SMALL[name]()
    a, v, _, tr = traced(name)
    assert v.sum() == 0
    cfg = R.full_cfg(sc["cfg"])
    n = len(sc["poses"]); c = sc["cand"]; e = sc["edges"]
    pos = R.positions(sc["poses"]); adj = R.adjacency(n, e)
    merged = np.zeros(n, np.uint8) if sc["merged"] is None else sc["merged"]
    key = lambda f, t, ty: (min(f, t), max(f, t), ty)
    exists = {key(f, t, ty) for f, t, ty in zip(e["from"].tolist(), e["to"].tolist(), e["type"].tolist()) if 0 <= f < n and 0 <= t < n}
    out = np.zeros(len(c), np.uint8)
    slots = 2
    for first in range(0, len(c), 256):
        chunk = range(first, min(first + 256, len(c)))
        grown = False
        for k in chunk:
            f, t, ty = int(c["from"][k]), int(c["to"][k]), int(c["type"][k])
            if not (0 <= f < n and 0 <= t < n) or merged[f] or merged[t] or key(f, t, ty) in exists:
                continue
            out[k] = 2 if slots == 2 else 3
            if R.thresholds_ok(cfg, float(c["matching_score"][k]), c["transform"][k].tolist()):
                peak = tr[k][2] if tr[k] is not None else R.astar(pos, adj, f, t)[2]
                out[k] = max(out[k], code_of(peak))
                grown = grown or peak > 128
        exists |= {key(int(c["from"][k]), int(c["to"][k]), int(c["type"][k])) for k in chunk if a[k]}
        slots = 4 if grown else slots
    return out


@pytest.mark.parametrize("name", sorted(S.SMALL))
def test_scene_equals_oracle(capi, oracle, name):
    sc = S.SMALL[name]()
    exp = expected(oracle, name, sc)
    g = capi.Gate(**sc["cfg"]); g.set_graph(sc["poses"], sc["edges"], sc["merged"])
    assert same(g.check(sc["cand"]), exp)
    assert g.edge_count() == exp[3]
    # a second call sees the edges the first one accepted (existsEdge) and accepts nothing.  (Not so in `chunks`, by the oracle itself:
    # its valid accepts of the whole first call lead the greedy search of 14 candidates rejected then onto longer paths, which pass.)
    a2, _, _ = g.check(sc["cand"])
    assert np.array_equal(a2, exp[4]) and a2.sum() == (14 if name == "chunks" else 0)
    g.close()
    g = capi.Gate(**sc["cfg"]); g.set_graph(sc["poses"], sc["edges"], sc["merged"])
    a, v, d = g.check(sc["cand"], want_dist=False)
    assert d is None and same((a, v, None), exp) and g.edge_count() == exp[3]
    g.close()


@pytest.mark.parametrize("name", ["stages", "stages_ssf0", "stages_ssfneg"])
def test_stage_rows_settle_where_the_reference_says(capi, oracle, name):
    sc = S.SMALL[name]()
    exp = expected(oracle, name, sc)
    adj = R.adjacency(len(sc["poses"]), sc["edges"])
    want = {row: R.stage(sc["cfg"], sc["poses"], adj, sc["cand"][k])["stage"] for k, row in enumerate(sc["rows"])}
    g = capi.DiagGate(**sc["cfg"]); g.set_graph(sc["poses"], sc["edges"], sc["merged"])
    a, v, d = g.check(sc["cand"], want_dist=False)
    st = dict(zip(sc["rows"], g.stages().tolist()))
    assert same((a, v, None), exp)
    for row in sc["rows"]:
        assert st[row] == (2 if want[row] == "search" else 1), (row, want[row], st)     # (every list here has one or two entries)
    if name == "stages":
        assert [st[r] for r in ("i", "ii", "iii", "vi", "vii", "viii")] == [1] * 6 and min(st[r] for r in ("iv", "v", "xi")) >= 2
    if name == "stages_ssfneg":
        assert min(st.values()) >= 2
    # asked for the distances, every candidate is searched
    g.set_graph(sc["poses"], sc["edges"], sc["merged"])
    assert same(g.check(sc["cand"]), exp) and g.stages().tolist() == [2] * len(sc["rows"])
    g.close()


def test_escalation_two_four_slots_then_the_lane_kernel(capi, oracle):
    sc = S.escalation()
    exp = expected(oracle, "escalation", sc)
    want = predicted("escalation")
    assert {2, 3, 5} <= set(want.tolist())
    g = capi.DiagGate(**sc["cfg"]); g.set_graph(sc["poses"], sc["edges"], sc["merged"])
    assert same(g.check(sc["cand"]), exp)
    assert np.array_equal(g.stages(), want)
    # the same searches under another edge type: the handle now starts with four entries per lane
    c2 = sc["cand"].copy(); c2["type"] = 9
    o = oracle.Gate(**sc["cfg"]); o.set_graph(sc["poses"], sc["edges"], sc["merged"]); o.check(sc["cand"])
    exp2 = o.check(c2); o.close()
    assert same(g.check(c2), exp2)
    st2 = g.stages()
    both = (exp2[2] != -1) & (want != 0)
    assert 2 not in st2 and np.array_equal(st2[both], np.maximum(want, 3)[both]) and (st2 == 3).sum() >= 4 and (st2 == 5).sum() >= 2
    g.close()


@pytest.mark.parametrize("name", SINGLE_PASS)
def test_no_search_falls_back_silently(capi, oracle, name):
    sc = S.SMALL[name]()
    exp = expected(oracle, name, sc)
    want = predicted(name)
    assert 5 not in want
    g = capi.DiagGate(**sc["cfg"]); g.set_graph(sc["poses"], sc["edges"], sc["merged"])
    assert same(g.check(sc["cand"]), exp)
    st = g.stages()
    searched = exp[2] != -1
    assert np.isin(st[searched], (2, 3)).all() and np.array_equal(st, want)
    g.close()
    # without the distances: the same verdicts, and what the deciding search leaves over goes to the same kernels
    g = capi.DiagGate(**sc["cfg"]); g.set_graph(sc["poses"], sc["edges"], sc["merged"])
    a, v, _ = g.check(sc["cand"], want_dist=False)
    st = g.stages()
    assert same((a, v, None), exp)
    assert np.array_equal(st == 0, want == 0) and np.isin(st[searched], (1, 2, 3)).all()
    g.close()


def test_chunks_replay_across_the_chunk_edge(capi, oracle):
    sc = S.chunks()
    exp = expected(oracle, "chunks", sc)
    ref = traced("chunks")
    assert same(ref[:3], exp)
    for want_dist in (True, False):
        g = capi.Gate(**sc["cfg"]); g.set_graph(sc["poses"], sc["edges"], sc["merged"])
        fresh = capi.Gate(**sc["cfg"]); fresh.set_graph(sc["poses"], sc["edges"], sc["merged"])
        got = g.check(sc["cand"], want_dist=want_dist); again = fresh.check(sc["cand"], want_dist=want_dist)
        assert same(got, exp) and same(again, exp)
        assert got[0][255] == 1 and got[1][255] == 1 and got[0][256] == 0
        assert g.edge_count() == fresh.edge_count() == exp[3]
        g.close(); fresh.close()


def _large(capi, oracle, n):
    sc = S.large(n)
    exp = expected(oracle, "large_%d" % n, sc)
    adj = R.CsrAdjacency(n, sc["edges"]); pos = sc["poses"][:, [3, 7, 11]]
    c = sc["cand"]
    peaks = [R.astar(pos, adj, int(c["from"][k]), int(c["to"][k]))[2] for k in range(len(c))]
    assert (exp[2] != -1).all() and (exp[2] == R.DMAX).sum() == 1 and 0 < exp[0].sum() < len(c)
    return sc, exp, peaks


def test_large_last_size_on_the_lds_path(capi, oracle):
    """n = 384 512: the closed / open bitmaps fill gate_reg_kernel's and gate_bound_kernel's dynamic LDS to exactly kGateLdsMax"""
    sc, exp, peaks = _large(capi, oracle, S.LARGE_LAST_LDS)
    g = capi.DiagGate(**sc["cfg"]); g.set_graph(sc["poses"], sc["edges"])
    assert same(g.check(sc["cand"]), exp) and g.edge_count() == exp[3]
    st = g.stages().tolist()
    assert st == [code_of(p) for p in peaks] and 4 not in st and {2, 3, 5} <= set(st)
    g.close()
    g = capi.DiagGate(**sc["cfg"]); g.set_graph(sc["poses"], sc["edges"])
    a, v, _ = g.check(sc["cand"], want_dist=False)
    assert same((a, v, None), exp) and 4 not in g.stages().tolist()
    g.close()


def test_large_first_size_on_the_wave_kernel(capi, oracle):
    """n = 384 513: one node more than the bitmaps hold - gate_wave_kernel searches, and hands the search that outgrows its 2 048
    entries to gate_kernel"""
    sc, exp, peaks = _large(capi, oracle, S.LARGE_FIRST_WAVE)
    g = capi.DiagGate(**sc["cfg"]); g.set_graph(sc["poses"], sc["edges"])
    assert same(g.check(sc["cand"]), exp) and g.edge_count() == exp[3]
    st = g.stages().tolist()
    assert st == [5 if p > 2048 else 4 for p in peaks] and st.count(5) == 1 and st[list(sc["rows"]).index("cluster")] == 5
    g.close()
    g = capi.DiagGate(**sc["cfg"]); g.set_graph(sc["poses"], sc["edges"])
    a, v, _ = g.check(sc["cand"], want_dist=False)
    assert same((a, v, None), exp)
    line = [R.line_decides(sc["cfg"], sc["poses"][int(f)].tolist(), sc["poses"][int(t)].tolist())[0] for f, t in zip(sc["cand"]["from"], sc["cand"]["to"])]
    st = g.stages().tolist()
    assert st == [1 if l else (5 if p > 2048 else 4) for l, p in zip(line, peaks)] and not all(line)      # nothing settled by the ball
    g.close()
