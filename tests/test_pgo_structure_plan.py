"""The structure of a pose graph (csrc/pgo_structure.hip) on the CPU, through uzl_debug_pgo_structure_plan of the diagnostic library
(capi.pgo_structure_plan): host integer work, no device.  Every comparison is integer array_equal against a reference that is not the
code under test: the oracle for the skip rules and the gauge, structure_reference.py - the rules restated from their comments - for the
rest.  A slip here is silent on the device: a slower or subtly different solve, not a failure."""
import os

import numpy as np
import pytest

import ml_classes as MC
import structure_reference as SR
import test_ml_plan as TM
from uzliti_slam_amd import capi, synth

plan = capi.pgo_structure_plan


@pytest.fixture(autouse=True)
def _needs_the_diagnostic_library():
    if not os.path.exists(capi.DIAG_LIB_PATH):
        pytest.skip("diagnostic library not built")


def flatten(g):
    ie, w = SR.in_edges_of(g)
    return plan("flatten", n=len(g["nodes_fixed"]), fixed=g["nodes_fixed"], in_edges=ie, in_w=w), ie, w


def chain(n, extra=()):
    return np.asarray([(i, i + 1) for i in range(n - 1)] + list(extra), np.int32).reshape(-1, 2)


def fixed0(n, which=(0,)):
    f = np.zeros(n, np.uint8); f[list(which)] = 1
    return f


# ------------------------------------------------------------------------------------------------------------------ flatten / gauge
def test_skip_rules_are_the_oracles(oracle):
    g = SR.skip_rule_graph()
    got, ie, w = flatten(g)
    ref = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    keep = ref["ij"][:, 0] != ref["ij"][:, 1]                # the one rule the library adds: a self edge is no constraint
    assert (~keep).sum() == 1
    assert np.array_equal(got["ij"], ref["ij"][keep]) and np.array_equal(got["src"], ref["src_edge"][keep])
    assert np.array_equal(got["robust"], ref["robust"][keep]) and np.array_equal(got["edge_w"], w[got["src"]])
    # the case is what it says: every kind of dropped edge is in the input, and its kept twin in the output
    last = len(ie) - 10 + np.arange(10)
    assert [int(k) in set(got["src"].tolist()) for k in last] == [False, False, False, False, True, False, True, False, True, True]
    odom = ie[got["src"], 2] != 0
    assert odom.any() and not odom[np.argmin(odom):].any()   # odometry edges first, then the feature edges
    assert np.array_equal(got["robust"], (~odom).astype(np.uint8))


@pytest.mark.parametrize("case", ["two free components", "fixed in the middle", "all fixed", "no edges", "skip rules"])
def test_gauge_is_the_oracles(oracle, case):
    n, fixed, ij = {"two free components": (9, fixed0(9, ()), chain(9)[[0, 1, 2, 4, 5, 6, 7]][:, ::-1]),      # 0-3 | 4-8, edges pointing backwards
                    "fixed in the middle": (7, fixed0(7, (3,)), chain(7)),
                    "all fixed": (5, np.ones(5, np.uint8), chain(5)),
                    "no edges": (4, fixed0(4, (2,)), chain(1))}.get(case) or (12, SR.skip_rule_graph()["nodes_fixed"], flatten(SR.skip_rule_graph())[0]["ij"])
    got = plan("gauge", n=n, fixed=fixed, ij=ij)
    want, cnt = oracle.set_fixed_nodes(fixed, ij)
    assert np.array_equal(got["fixed_eff"], want) and got["n_gauge"] == cnt
    assert cnt == {"two free components": 2, "fixed in the middle": 0, "all fixed": 0, "no edges": 3}.get(case, cnt)
    if case == "two free components":
        assert got["fixed_eff"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 0]          # the lowest index of each component
    # and the block system of what is left: nb = 0 when every vertex is fixed, no slot without an edge
    b2v = plan("order", n=n, fixed=got["fixed_eff"], ij=ij)["b2v"]
    Y = plan("system", n=n, ij=ij, robust=np.zeros(len(ij), np.uint8), b2v=b2v)
    assert Y["nb"] == n - int(got["fixed_eff"].sum()) == len(b2v)
    if case == "all fixed":
        assert (Y["nb"], Y["nslots"], Y["row_ptr"].tolist(), Y["rb_ptr"].tolist()) == (0, 0, [0], [0, 0]) and (Y["rowhdr"] == -1).all()
    if case == "no edges":
        assert got["fixed_eff"].all() and Y["nslots"] == 0 and Y["row_ptr"].tolist() == [0]          # every vertex is a component of its own


# ------------------------------------------------------------------------------------------------------------------ order
MIDDLE = np.r_[12:24, 0:12]              # a path through the vertices in this order: the walk starts at vertex 0, in its middle


def order_cases():
    n = 24
    ij = chain(n, [(3, 17), (8, 20)])
    w = np.concatenate([np.full(n - 1, 100.0), [10.0, 10.0]])
    perm = np.random.default_rng(7).permutation(n)
    out = {"time-ordered chain": (n, fixed0(n), ij, w), "permuted chain": (n, fixed0(n)[np.argsort(perm)], perm[ij].astype(np.int32), w),
           "start in the middle": (n, fixed0(n, ()), np.stack([MIDDLE[:-1], MIDDLE[1:]], 1).astype(np.int32), None)}
    # a weight tie goes to the lower index: vertex 1's neighbours 5 and 2 weigh the same
    out["weight tie"] = (6, fixed0(6), np.asarray([(0, 1), (1, 5), (1, 2), (2, 3), (3, 4), (4, 5)], np.int32), np.asarray([1.0, 7.0, 7.0, 7.0, 7.0, 7.0]))
    ga, gb = synth.make_pose_graph(20, 30, seed=1), synth.make_pose_graph(20, 30, seed=2)
    g = synth.interleave_sessions(ga, gb, n_cross=6)
    F, _, _ = flatten(g)
    fe = plan("gauge", n=40, fixed=g["nodes_fixed"], ij=F["ij"])["fixed_eff"]
    out["interleaved sessions"] = (40, fe, F["ij"], F["edge_w"])
    return out


@pytest.mark.parametrize("case", ["time-ordered chain", "permuted chain", "start in the middle", "weight tie", "interleaved sessions"])
def test_aggregation_order(case):
    n, fixed, ij, w = order_cases()[case]
    got = plan("order", n=n, fixed=fixed, ij=ij, edge_w=w)["b2v"]
    assert np.array_equal(got, SR.aggregation_order(n, ij, fixed, w))
    assert sorted(got.tolist()) == np.nonzero(fixed == 0)[0].tolist()
    if case == "time-ordered chain":
        assert np.array_equal(got, np.arange(1, n))                              # index order: nothing changes for a single session
    if case == "permuted chain":
        inv = np.argsort(np.random.default_rng(7).permutation(n))
        assert np.all(np.abs(np.diff(inv[got])) == 1)                            # the trajectory again (from either end), whatever the ids
    if case == "start in the middle":                                            # vertex 0 sits in the middle of the path: backward extension
        assert np.array_equal(got, MIDDLE)
    if case == "weight tie":
        assert got.tolist() == [1, 2, 3, 4, 5]
    if case == "interleaved sessions":
        sess = got % 2                                                           # ids interleave a0 b0 a1 b1: the order follows each session's chain
        assert (np.diff(sess) != 0).sum() <= 6 and (np.diff(np.arange(40)[fixed == 0] % 2) != 0).sum() > 30


# ------------------------------------------------------------------------------------------------------------------ block-CSR
def system_cases():
    out = {}
    # multi-edges (three slots for one block, both directions), a fixed neighbour, robust flags
    ij = np.asarray([(0, 1), (1, 2), (2, 1), (1, 2), (2, 3), (3, 0), (3, 1)], np.int32)
    out["multi-edges"] = (4, fixed0(4), ij, np.asarray([0, 0, 1, 1, 0, 1, 1], np.uint8), None)
    out["order given"] = (4, fixed0(4), ij, np.asarray([0, 0, 1, 1, 0, 1, 1], np.uint8), np.asarray([3, 1, 2], np.int32))
    for k in (20, 21):                                       # a row with exactly k neighbours: the row header holds 20
        n = k + 2
        out["%d neighbours" % k] = (n, fixed0(n), np.asarray([(0, 1)] + [(1, 2 + i) if i % 2 else (2 + i, 1) for i in range(k - 1)], np.int32),
                                    np.ones(k, np.uint8), None)
    return out


@pytest.mark.parametrize("case", ["multi-edges", "order given", "20 neighbours", "21 neighbours"])
def test_block_csr(case):
    n, fixed, ij, robust, b2v = system_cases()[case]
    if b2v is None:
        b2v = plan("order", n=n, fixed=fixed, ij=ij)["b2v"]
    got = plan("system", n=n, ij=ij, robust=robust, b2v=b2v)
    want = SR.block_csr(n, ij, robust, b2v)
    for k in ("nb", "nslots"):
        assert got[k] == want[k]
    for k in ("v2b", "row_ptr", "col", "slot_edge", "smeta"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["rowhdr"], SR.row_headers(want["row_ptr"], want["col"]))
    assert np.array_equal(got["rb_ptr"], SR.row_blocks(want["row_ptr"])) and got["n_rb"] == len(got["rb_ptr"]) - 1
    if np.array_equal(b2v, np.nonzero(fixed == 0)[0]):                           # index order: test_ml_plan.csr itself
        rp, col = TM.csr(n, ij, fixed=np.nonzero(fixed)[0])
        assert np.array_equal(got["row_ptr"], rp) and np.array_equal(got["col"], col)
    rp, se, sm = got["row_ptr"], got["slot_edge"], got["smeta"]
    for a in range(got["nb"]):                                                   # slot order = edge order within a row
        assert np.all(np.diff(se[rp[a]:rp[a + 1]] >> 1) > 0) or case in ("multi-edges", "order given")
        assert np.all(np.diff(se[rp[a]:rp[a + 1]] >> 1) >= 0)
    partner = (sm[:, 3] & ~(1 << 30)) - 1
    for q in np.nonzero(partner >= 0)[0]:                                        # the partner slot is the same edge seen from its other end
        assert se[partner[q]] == se[q] ^ 1 and got["col"][q] >= 0
    assert np.array_equal(partner < 0, got["col"] < 0) and np.array_equal(sm[:, 3] >> 30, robust[se >> 1])
    if case == "multi-edges":
        assert (got["col"][rp[0]:rp[1]] == 1).sum() == 3 and got["col"][rp[0]] == -1          # row of vertex 1: fixed neighbour first, block (1, 2) three times
    if case.endswith("neighbours"):
        k, a = int(case.split()[0]), got["v2b"][1]                               # the hub is vertex 1
        hdr = got["rowhdr"][a]
        assert rp[a + 1] - rp[a] == k and (hdr[0], hdr[1]) == (rp[a], rp[a + 1]) and np.array_equal(hdr[2:22], got["col"][rp[a]:rp[a] + 20])
        assert (hdr[2:22] != -1).sum() == 19 and np.all(got["rowhdr"][:, 22:] == -1)          # (the first of the 20 is the fixed vertex 0: -1)


# ------------------------------------------------------------------------------------------------------------------ row blocks
def rows_of(degrees):
    return np.concatenate([[0], np.cumsum(degrees)]).astype(np.int32)


def smallest_above(cap_of, limit):
    """the smallest argument at which cap_of first exceeds limit (cap_of is monotone): by bisection on the restated formula"""
    lo, hi = 0, 1 << 30
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if cap_of(mid) > limit else (mid, hi)
    return hi


def row_block_cases():
    out = {"42 rows": rows_of([2] * 42), "43 rows": rows_of([2] * 43), "256 slots": rows_of([8] * 32), "257 slots": rows_of([8] * 31 + [9]),
           "hub of 300": rows_of([3] * 10 + [300] + [3] * 10), "empty": rows_of([])}
    # the caps grow beyond kMaxPartials / 2 blocks' worth: one below and at the first size where each exceeds its floor
    ns = smallest_above(lambda s: SR.row_caps(1, s)[0], 256)
    nb = smallest_above(lambda r: SR.row_caps(r, 0)[1], 42)
    assert (ns, nb) == (256 * (MC.MAX_PARTIALS // 2) + 1, 42 * (MC.MAX_PARTIALS // 2) + 1)
    for name, slots in (("slot cap below", ns - 1), ("slot cap at", ns)):
        d = np.full(slots // 8, 8); d[0] += slots - d.sum()                      # rows of 8 slots: 32 rows fill a block of 256
        out[name] = rows_of(d)
    for name, rows in (("row cap below", nb - 1), ("row cap at", nb)):
        out[name] = rows_of(np.ones(rows, np.int64))
    return out


@pytest.mark.parametrize("case", ["42 rows", "43 rows", "256 slots", "257 slots", "hub of 300", "empty", "slot cap below", "slot cap at", "row cap below",
                                  "row cap at"])
def test_row_blocks(case):
    rp = row_block_cases()[case]
    nb = len(rp) - 1
    got = plan("row_blocks", row_ptr=rp)
    rb = got["rb_ptr"]
    assert got["max_partials"] == MC.MAX_PARTIALS and (got["cap_slots"], got["cap_rows"]) == SR.row_caps(nb, int(rp[nb]))
    assert np.array_equal(rb, SR.row_blocks(rp))
    assert rb[0] == 0 and rb[-1] == nb and (np.all(np.diff(rb) > 0) or nb == 0) and len(rb) - 1 <= MC.MAX_PARTIALS          # the blocks tile [0, nb)
    want = {"42 rows": [0, 42], "43 rows": [0, 42, 43], "256 slots": [0, 32], "257 slots": [0, 31, 32], "hub of 300": [0, 10, 11, 21], "empty": [0, 0]}
    if case in want:
        assert rb.tolist() == want[case]
    caps = {"slot cap below": (256, 42), "slot cap at": (512, 42), "row cap below": (256, 42), "row cap at": (256, 43)}
    if case in caps:
        assert (got["cap_slots"], got["cap_rows"]) == caps[case]


# ------------------------------------------------------------------------------------------------------------------ numbering ladder
HISTORY = {"none": (-1.0, -1.0), "row only, 40": (40.0, -1.0), "row only, above 40": (40.5, -1.0), "strong only, 40": (-1.0, 40.0),
           "strong only, above 40": (-1.0, 40.5), "both, strong cheaper": (30.0, 29.5), "both, equal": (30.0, 30.0), "both, row cheaper": (29.0, 30.0)}


@pytest.mark.parametrize("cfg", [0, 1, 2])
@pytest.mark.parametrize("history", list(HISTORY))
def test_numbering_ladder(cfg, history):
    for pre, shard in ((1, False), (1, True), (0, False)):
        got = plan("numbering", cfg_numbering=cfg, preconditioner=pre, may_shard=shard, num_its=HISTORY[history])
        assert (got["strong_min"], got["max_contig"]) == SR.reduced_numbering(cfg, pre, shard, HISTORY[history]), (pre, shard)
        if shard or pre == 0 or cfg == 1:
            assert got["strong_min"] == 0
    got = plan("numbering", cfg_numbering=cfg, preconditioner=1, may_shard=False, num_its=HISTORY[history])
    pinned = {(0, "none"): (32, 0.6), (0, "row only, 40"): (0, 2.0), (0, "row only, above 40"): (32, 2.0), (0, "strong only, 40"): (32, 2.0),
              (0, "strong only, above 40"): (0, 2.0), (0, "both, equal"): (0, 2.0), (0, "both, strong cheaper"): (32, 2.0), (2, "both, row cheaper"): (32, 2.0)}
    if (cfg, history) in pinned:
        assert (got["strong_min"], got["max_contig"]) == pinned[(cfg, history)]


# ------------------------------------------------------------------------------------------------------------------ Schur admission
def test_schur_admission_at_its_two_thresholds():
    for nb, n_int in ((100, 63), (100, 64), (191, 63), (191, 64), (200, 65), (200, 66), (1000, 329), (1000, 330), (1001, 330), (1001, 331), (0, 0)):
        got = plan("admission", nb=nb, n_int=n_int)
        assert got["admitted"] == SR.schur_admitted(nb, n_int) and got["min_int"] == SR.schur_min_int(nb), (nb, n_int)
        assert got["admitted"] == (n_int >= got["min_int"])                      # min_int is the cut itself, rounding included
    assert [plan("admission", nb=nb, n_int=k)["admitted"] for nb, k in ((100, 63), (100, 64), (1000, 329), (1000, 330), (200, 65), (200, 66))] == \
        [False, True, False, True, False, True]                                 # 63 | 64 rows; 32.9 % | 33 %; 32.5 % | 33 %


# ------------------------------------------------------------------------------------------------------------------ shard range
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_ranges_tile_the_edges(world):
    for e in (0, 1, 7, 8, 9):
        got = [plan("shard", e=e, rank=r, world=world) for r in range(world)]
        assert [(g["e_begin"], g["e_end"], g["diag_owner"]) for g in got] == [SR.shard_range(e, r, world) for r in range(world)]
        assert got[0]["e_begin"] == 0 and got[-1]["e_end"] == e and all(a["e_end"] == b["e_begin"] for a, b in zip(got, got[1:]))
        sizes = [g["e_end"] - g["e_begin"] for g in got]
        assert max(sizes) - min(sizes) <= 1 and [g["diag_owner"] for g in got] == [1] + [0] * (world - 1)


# ------------------------------------------------------------------------------------------------------------------ exchange layout
@pytest.mark.parametrize("nb,make,flags,gather", [(8, TM.loopy, {}, 0), (999, TM.loopy, {}, 1), (3073, TM.loopy, {}, 2), (4097, TM.sparse, {}, 2),
                                                  (999, TM.loopy, dict(precond_on=False), 0)])
def test_exchange_layout(nb, make, flags, gather):
    rp, col = make(nb)
    P = capi.ml_plan(rp, col, arrays=False, **flags)
    got = plan("exchange", row_ptr=rp, col=col, **flags)
    want = SR.exchange_layout(nb, P)
    assert got["gather_level"] == (P["gather_level"] if P["levels"] else 0) == gather
    assert {k: got[k] for k in want} == want
    n_g = P["lv"][gather]["n"] if gather else 0
    assert got["n_gather"] == n_g and got["part_a"] - got["sg"] == 6 * n_g * (2 if gather == 2 else 1)          # level 2 doubles the span
    assert got["iter_span"] - got["part_a"] <= MC.MAX_PARTIALS and got["part_a"] <= 12 * max(nb, 1)            # inside SysBufs::ap [12 nb + kMaxPartials]


# ------------------------------------------------------------------------------------------------------------------ growth test
def grown_cases():
    n = 40
    ij = chain(n, [(i, i + 20) for i in range(0, 20, 2)] + [(39, 0)])          # 50 edges
    f = fixed0(n)
    old = (n, f, ij)
    more = np.concatenate([ij[:39], [(40, 41)], ij[39:], [(41, 42), (3, 42)]]).astype(np.int32)
    out = {"unchanged": (old, old, True), "appended": (old, (43, fixed0(43), more), True),
           "nine in ten survive": (old, (n, f, np.delete(ij, [4, 11, 23, 30, 47], 0)), True),
           "one fewer": (old, (n, f, np.delete(ij, [4, 11, 23, 30, 47, 48], 0)), False),
           "fewer nodes": ((n, f, ij[:38]), (39, fixed0(39), ij[:38]), False),
           "fixed prefix changed": (old, (n, fixed0(n, (0, 7)), ij), False),
           "new nodes' flags are free": (old, (43, fixed0(43, (0, 41)), more), True),
           "unrelated": (old, (n, f, np.random.default_rng(3).integers(0, n, (50, 2)).astype(np.int32)), False),
           "no old edges": ((n, f, ij[:0]), old, True)}
    return out


@pytest.mark.parametrize("case", list(grown_cases()))
def test_graph_grown(case):
    old, new, want = grown_cases()[case]
    got = plan("grown", old=old, new=new)
    assert got["grown"] == SR.graph_grown(old, new) == want
    assert got["survive"] == SR.edges_survive_in_order(old[2], new[2])


def test_early_exit_equals_the_plain_loop():
    """200 random old / new pairs around the nine-in-ten boundary and far from it, windows 8 and 4096: the early exit changes no verdict"""
    rng = np.random.default_rng(11)
    verdicts = []
    for trial in range(200):
        e = int(rng.integers(100, 400))
        old = rng.integers(0, 60, (e, 2)).astype(np.int32)
        drop = rng.random(e) < (0.5 if trial % 4 == 0 else rng.uniform(0.05, 0.15))
        new = old[~drop]
        ins = rng.integers(0, 60, (int(rng.integers(0, 30)), 2)).astype(np.int32)
        at = np.sort(rng.integers(0, len(new) + 1, len(ins)))
        new = np.insert(new, at, ins, 0) if trial % 3 else (rng.integers(0, 60, (e, 2)).astype(np.int32) if trial % 2 else new)
        for window in (8, 4096):
            got = plan("grown", old=(60, np.zeros(60, np.uint8), old), new=(60, np.zeros(60, np.uint8), new), window=window)
            want = SR.edges_survive_in_order(old, new, window)
            assert got["survive"] == want == got["grown"], (trial, window)
            verdicts.append(want)
    assert 0.2 < np.mean(verdicts) < 0.8                                         # both verdicts are exercised


# ------------------------------------------------------------------------------------------------------------------ determinism
def test_two_calls_give_the_same_bytes():
    g = synth.interleave_sessions(synth.make_pose_graph(20, 30, seed=1), synth.make_pose_graph(20, 30, seed=2), n_cross=6)
    runs = []
    for _ in range(2):
        F, _, _ = flatten({k: (np.array(v) if not isinstance(v, dict) else {a: np.array(b) for a, b in v.items()}) for k, v in g.items()})
        G = plan("gauge", n=40, fixed=g["nodes_fixed"], ij=F["ij"])
        b2v = plan("order", n=40, fixed=G["fixed_eff"], ij=F["ij"], edge_w=F["edge_w"])["b2v"]
        Y = plan("system", n=40, ij=F["ij"], robust=F["robust"], b2v=b2v)
        runs.append([F[k].tobytes() for k in ("ij", "src", "robust", "edge_w")] + [G["fixed_eff"].tobytes(), b2v.tobytes()] +
                    [Y[k].tobytes() for k in ("v2b", "row_ptr", "col", "slot_edge", "smeta", "rb_ptr", "rowhdr")])
    assert runs[0] == runs[1]
