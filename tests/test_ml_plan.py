"""The hierarchy plan (csrc/pgo_ml_plan.hip: ml_plan) on the CPU, through uzl_debug_ml_plan of the diagnostic library (capi.ml_plan): host
integer work, no device.

  structure      hierarchy_checks.check_structure - the check test_pgo_hierarchy_gpu.py makes on the device's hierarchy - on the plan of
                 every graph shape that module uses: the coarse levels against np_reference.ml_coarse_structure
  class table    at every boundary where the class changes, against ml_classes.expected_class: the rules restated in Python, not the code
                 under test.  A slip here is silent on the device and costs a 2-5x slower solve.
  determinism    two calls, byte-equal arrays

Block-Jacobi is levels = 0; what the plan holds besides (agg keeps the value the rules gave it when the LDS admission fails) is not read by
anything and not asserted."""
import os

import numpy as np
import pytest

import hierarchy_checks as HC
import ml_classes as MC
from uzliti_slam_amd import capi, synth


@pytest.fixture(autouse=True)
def _needs_the_diagnostic_library():
    if not os.path.exists(capi.DIAG_LIB_PATH):
        pytest.skip("diagnostic library not built")


def csr(n, edges, fixed=(0,)):
    """test_schur_plan._csr with arrays: block-CSR over the free vertices as uzl_pgo builds it - one slot per (free endpoint, edge) in edge
    order, col = -1 for a fixed neighbour."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    free = np.ones(n, bool); free[list(fixed)] = False
    v2b = np.where(free, np.cumsum(free) - 1, -1)
    row = v2b[edges].reshape(-1)                              # slot 2k: edge k in its first endpoint's row; 2k + 1: in its second's
    col = v2b[edges[:, ::-1]].reshape(-1)
    keep = row >= 0
    row, col = row[keep], col[keep]
    order = np.argsort(row, kind="stable")
    rp = np.zeros(int(free.sum()) + 1, np.int32)
    np.cumsum(np.bincount(row, minlength=len(rp) - 1), out=rp[1:])
    return rp, col[order].astype(np.int32)


def chain_csr(nb, closures, seed):
    """nb free vertices behind one fixed vertex: the odometry chain and `closures` random loop closures."""
    rng = np.random.default_rng(seed)
    n = nb + 1
    a = rng.integers(0, n, closures); b = rng.integers(0, n, closures)
    ok = a != b
    chain = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    return csr(n, np.concatenate([chain, np.stack([a[ok], b[ok]], 1)]))


# ------------------------------------------------------------------------------------------------------------------ structure
# (nodes, edges, seed) of test_pgo_hierarchy_gpu.py: one coarse level, dense level 1 (DENSE1, the short last aggregates), dense level 2,
# the per-level geometry sizes, the reduced system of 1500 / 1530 in row order (its block-CSR: the Schur plan's)
SHAPES = ([(10, 20, 8)] + [(nb + 1, 3 * (nb + 1), nb) for nb in (9, 59, 64)] + [(nb + 1, e, 2 if nb == 999 else nb) for nb, e in MC.DENSE1] +
          [(nb + 1, 3 * nb, nb) for nb in range(201, 208)] + [(3074, 12300, 3073), (4000, 16000, 40), (5000, 5600, 50), (10000, 50000, 4),
                                                              (14000, 60000, 4)])


def graph_csr(nodes, e, seed):
    g = synth.make_pose_graph(nodes, e, seed=seed)
    ed = g["edges"]
    return csr(nodes, np.stack([np.asarray(ed["from"]), np.asarray(ed["to"])], 1), fixed=np.nonzero(np.asarray(g["nodes_fixed"]))[0])


@pytest.mark.parametrize("nodes,e,seed", SHAPES)
def test_coarse_structure_is_the_references(nodes, e, seed):
    rp, col = graph_csr(nodes, e, seed)
    for flags in ({}, dict(comp4_off=True)) if nodes >= 4000 else ({},):
        h = capi.ml_plan(rp, col, **flags)
        want = MC.expected_class(len(rp) - 1, len(col), **flags)
        assert h["levels"] == want["levels"] and (h["levels"] == 0 or [lv["n"] for lv in h["lv"]] == want["n"])
        HC.check_structure(h)


def test_coarse_structure_of_a_reduced_system():
    rp, col = graph_csr(1500, 1530, 15)
    red = capi.schur_plan(rp, col, 24)
    assert 64 < red["n_reduced"] < len(rp) - 1
    h = capi.ml_plan(red["row_ptr"], red["col"])
    assert h["levels"] >= 2 and h["agg"] == 1 and h["cl"] == 1
    HC.check_structure(h)


# ------------------------------------------------------------------------------------------------------------------ class table
def loopy(nb):
    return chain_csr(nb, 3 * nb, nb)             # ~ 8 slots per row: nslots >= 6 nb


def sparse(nb):
    return chain_csr(nb, nb // 8, nb)            # ~ 2.25 slots per row


# (case, CSR maker, free vertices, flags, what the case is there for - asserted besides the table)
CASES = [("8 rows", loopy, 8, {}, dict(levels=0)), ("9 rows", loopy, 9, {}, dict(levels=1, agg=1, cl=0, mult=0)),
         ("preconditioner off", loopy, 999, dict(precond_on=False), dict(levels=0)),
         ("64: one level", loopy, 64, {}, dict(levels=1, cl=0)), ("65: two levels", loopy, 65, {}, dict(levels=2, cl=1, mult=1, ns_steps=2)),
         ("1024: top of 16", loopy, 1024, {}, dict(levels=2, n=[1024, 128, 16])), ("1025: 17 adds a level", loopy, 1025, {}, dict(levels=3, n=[1025, 129, 17, 3])),
         ("3072 loopy", loopy, 3072, {}, dict(agg=1, cl=1, gather_level=1, ns_steps=2)),
         ("3073 loopy", loopy, 3073, {}, dict(agg=4, cl=2, gather_level=2, ns_steps=4)),
         ("3073 sparse", sparse, 3073, {}, dict(agg=1, cl=1)),
         ("4096 sparse", sparse, 4096, {}, dict(agg=1, cl=1, ns_steps=2)), ("4097 sparse", sparse, 4097, {}, dict(agg=4, cl=2, ns_steps=2)),
         ("strong blocks", sparse, 999, dict(strong_blocks=True), dict(agg=4, cl=2, gather_level=2)),
         ("strong blocks, two levels", sparse, 200, dict(strong_blocks=True), dict(agg=4, cl=0, levels=2, mult=0, gather_level=2)),
         ("mult banned, dense 1", loopy, 999, dict(mult_banned=True), dict(cl=1, mult=0, ns_steps=0)),
         ("mult banned, dense 2", loopy, 4000, dict(mult_banned=True), dict(cl=2, mult=0, ns_steps=0)),
         ("comp4 off", loopy, 10000, dict(comp4_off=True), dict(agg=4, cl=0, mult=0, ns_steps=0, gather_level=2)),
         ("comp4 off does not touch agg 1", loopy, 999, dict(comp4_off=True), dict(agg=1, cl=1, mult=1)),
         ("95520: n_2 = 2985", loopy, 95520, {}, dict(agg=4, cl=2, lds=48 * 2985 + 64)), ("95521: n_2 = 2986", loopy, 95521, {}, dict(levels=0))]


@pytest.mark.parametrize("case", [c[0] for c in CASES])
def test_class_at_the_boundaries(case):
    _, make, nb, flags, pinned = next(c for c in CASES if c[0] == case)
    rp, col = make(nb)
    assert len(rp) - 1 == nb and ((len(col) >= 6 * nb) == (make is loopy))
    want = MC.expected_class(nb, len(col), **flags)
    for k, v in pinned.items():
        assert want[k] == v, "the restated rules do not put %s where the case expects it: %s = %s" % (case, k, want[k])
    h = capi.ml_plan(rp, col, arrays=False, **flags)
    assert h["levels"] == want["levels"], (case, h["levels"], want["levels"])
    if want["levels"] == 0:
        return
    got = dict(h, n=[lv["n"] for lv in h["lv"]], fan=[lv["fan"] for lv in h["lv"]])
    for k, v in want.items():
        assert got[k] == v, "%s: %s = %s, the rules say %s" % (case, k, got[k], v)
    assert h["lds"] <= MC.LDS_LIMIT and h["lv"][0]["nslots"] == len(col)


def test_lds_boundary_is_the_gather_level_vectors():
    """48 n_2 + 64 <= 140 KiB ends at n_2 = 2985 (test_ml_admission.py): the restated rules agree, before the plan is asked."""
    assert 48 * 2985 + 64 <= MC.LDS_LIMIT < 48 * 2986 + 64
    assert -(-(-(-95520 // 8)) // 4) == 2985 and -(-(-(-95521 // 8)) // 4) == 2986


# ------------------------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("nb,make", [(999, loopy), (4097, sparse), (10000, loopy)])
def test_two_calls_give_the_same_bytes(nb, make):
    rp, col = make(nb)
    a, b = capi.ml_plan(rp, col), capi.ml_plan(rp.copy(), col.copy())
    assert {k: v for k, v in a.items() if k != "lv"} == {k: v for k, v in b.items() if k != "lv"}
    for x, y in zip(a["lv"], b["lv"]):
        assert (x["n"], x["fan"], x["nslots"]) == (y["n"], y["fan"], y["nslots"])
        assert x["row_ptr"].tobytes() == y["row_ptr"].tobytes() and x["col"].tobytes() == y["col"].tobytes()
