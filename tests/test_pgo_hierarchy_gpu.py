"""The multilevel preconditioner stage by stage against float64 (uzl_debug_pgo_hierarchy of the diagnostic library,
capi.DiagPgo.hierarchy; the checks themselves are hierarchy_checks.py, the reference np_reference.ml_*).

test_pgo_system_gpu.py pins H, the SpMV, the Schur complement and whole solves; of M^-1 it knows "the PCG converged", which any
SPD-ish operator achieves.  Here every set-up kernel's OUTPUT is compared with the float64 reference applied to that kernel's INPUTS as
the device holds them (the dumped arrays of the level below / the level above), so a failure names one stage, one level and one entry:

  structure (ml_plan)                       exact
  geometry (ml_geometry, both forms)        C_H eps (|t|_max + |c|); weights exact; EMPTY rows zero
  Galerkin (ml_galerkin)                    C_H eps |P|^T |A_l| |P|
  sibling / top inverses                    C_H eps |W|_2 |row i of W^-1|_2 |column j of W^-1|_2 (hierarchy_checks.inverse_bound);
                                            padded children: identity, bit-exact
  additive dense (ml_dense_level)           C_H eps (|S| + |P| |Y_{l+1}| |P|^T)
  multiplicative cycle X_0                  C_H eps (2 |S| + |S| |A| |S| + |Q| |Y| |Q|^T), |Q| = |P| + |S| |A| |P|
  Newton-Schulz at cl                       from the device's own X_0 (the hook asked for 0 steps); C_H eps sum_k (2 |X| + |X| |A| |X|)
  cycle + upper_ns steps above cl           one stage from the dumped Y_{l+1}, the two bounds added
  f32 copy (ml_cmat32 / GEMM epilogue)      bit for bit, pad columns zero
  application, first step (apply(op = 1))   C_H eps x the absolute-value application of |x|, from the dumped Winv, geo, Cmat32, top_inv

What the dense kernels compute, as the reference states it: the tiles on and above the diagonal, mirrored below (64 x 64 in
ml_mult_qyqt, 32 x 32 in both Newton-Schulz GEMMs), and a Newton-Schulz step as 2 X - X^T (A X) - the GEMMs read their left factor as
X[k][row].  For a symmetric X that is 2 X - X A X; the Gauss-Jordan sibling inverses, and with them X_0, are symmetric only to
eps kappa(W), far above C_H eps of a product, so which half counts is part of the result (hierarchy_checks.CYCLE_TILE / NS_TILE,
np_reference.ml_newton_schulz).  The mirror images are asserted bit for bit.

C_H = 1e3 (test_pgo_system_gpu.py); no other tolerance.  test_np_reference_system.py shows on the CPU that a dropped Galerkin
contribution, a centroid over fan, a sibling coupling left out of W, a transposed sibling tile, a skipped Newton-Schulz step and a
missing 16 x 16 tile of Q Y Q^T each exceed these bounds by >= 1e8.

Every case asserts the class ml_plan gave it (levels, cl, agg, mult, step count, sizes per level) - a case that falls to another path
fails, the ml_cg variant included (cg_variant).  Every case runs at lambda = lambda_init and 1e3 max diag; poses after optimize(5) once
per class.  The 4-step refinement production takes at the composite level from LM iteration 2 on is held against the reference on
4000 / 16000.

  steady state (ml_spmv, ml_alpha, ml_cg)   after k = 1, 2, 3, 7 iterations, every ml_cg variant: gather-level residual = P^T r; z = M^-1 r
                                            within the application bound + the coarse application of the recurrence drift
                                            C_R eps (k + 1) (|A| |x| + |b|); the direction p = z + beta p_old

  PCG iteration counts (pcg_stop = 1)       the device's count against a float64 PCG with the float64 reference operator

The spectrum of the whole operator against the reference application's is test_pgo_system_gpu.py's
(test_spectrum_extremes_are_the_reference_operators).

Measured on an MI355X (pytest -s prints the MEASURED table; worst ratio to the bound over every case of the module):
  geometry cen / d / R^T                    0 / 0 / 1.0e-3 (the centroids and offsets came out bit for bit the reference's)
  Galerkin blk / G / M                      3.2e-3 / 1.9e-3 / 2.8e-3 (C4 level 1; strong blocks level 2; 3072 level 1)
  sibling inverses / top inverse            5.0e-3 (nb = 205) / 3.1e-3 (C2)
  additive dense                            2.6e-3 (513)
  multiplicative cycle X_0                  4.5e-3 (3072)
  Newton-Schulz at cl / cycle + steps above 5.7e-3 (4000 / 16000 after optimize(5); its 4 steps: 2.0e-2) / 1.7e-3 (C4 level 3)
  f32 copy                                  exact
  application, first step                   2.5e-2 (nb = 9); walked hierarchy 2.8e-3
  steady state: rg / z / r - (b - A x) / p  1.5e-3 (C2, k = 3) / 6.1e-5 / 7.2e-3 (walked C4, k = 7) / 9.6e-4 (C4, k = 3)
  PCG iterations, device | reference with f32 Y_cl | with f64 Y_cl (pcg_stop = 1, pcg_tol 1e-7, lambda_init):
      513: 36 | 36 | 36     C2: 38 | 38 | 38     4000 / 16000: 79 | 79 | 79     1500 / 1530 reduced: 28 | 28 | 28
The module takes 22 s on 16 cores (the dense float64 products of the 3072-vertex case, 6 n_1 = 2304, are 2 s of it).
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hierarchy_checks as HC
import np_reference as NP
from ml_classes import DENSE1, levels1 as _levels1, levels4 as _levels4      # the class rules restated (shared with test_ml_plan.py)
from uzliti_slam_amd import synth

pytestmark = pytest.mark.gpu

MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nMEASURED (stage / worst ratio to its bound):")
        for k in sorted(MEASURED):
            print("  %-60s %.3e   (%s)" % (k, MEASURED[k][0], MEASURED[k][1]))


def _note(key, v, where):
    if key not in MEASURED or v > MEASURED[key][0]:
        MEASURED[key] = (float(v), where)


def _judge(findings, case):
    for f in findings:
        _note(f.stage, f.ratio, "%s level %d" % (case, f.level))
    bad = [f for f in findings if not f.ratio <= 1.0]
    assert not bad, "%s: %s" % (case, "; ".join("%s level %d entry %s: %.3g x its bound" % (f.stage, f.level, f.where, f.ratio) for f in bad))


def rows_poses(h, lin):
    """Translations (NaN: EMPTY row) and rotations of the system's rows, from the poses the hook linearised at."""
    P = lin["poses"].reshape(-1, 3, 4)
    b2v = h["b2v"]
    live = b2v >= 0
    t = np.full((len(b2v), 3), np.nan); R = np.tile(np.eye(3), (len(b2v), 1, 1))
    t[live] = P[b2v[live], :, 3]; R[live] = P[b2v[live], :, :3]
    return t, R


def check_setup(p, lin, lam, case, want):
    """Every set-up stage of one hierarchy at one lambda; returns the hierarchy."""
    h = p.hierarchy(lam)
    for k, v in want.items():
        got = [lv["n"] for lv in h["lv"]] if k == "n" else h[k]
        assert got == v, "%s is not the class it claims: %s = %s, expected %s" % (case, k, got, v)
    HC.check_structure(h)
    t, R = rows_poses(h, lin)
    _judge(HC.check_geometry(h, t, R), case)
    _judge(HC.check_galerkin(h), case)
    _judge(HC.check_inverses(h), case)
    h0 = None
    if h["mult"]:
        h0 = p.hierarchy(lam, 0)
        assert h0["ns_steps"] == 0 and h0["lam"] == h["lam"]
        for l in range(h["levels"]):                                     # the same set-up up to the steps: same inputs, bit for bit
            assert np.array_equal(h0["lv"][l]["Winv"], h["lv"][l]["Winv"]) and np.array_equal(h0["lv"][l]["geo"], h["lv"][l]["geo"])
        HC.check_cmat32(h0)
    _judge(HC.check_dense(h, h0), case)
    HC.check_cmat32(h)
    return h


def check_application(p, h, lam, case):
    """First PCG step z = M^-1 x: 3 random x and the 6 rigid-body modes of one aggregate."""
    rng = np.random.default_rng(h["rows"])
    n = h["rows"]
    xs = [rng.normal(size=(n, 6)) for _ in range(3)]
    A = (h["lv"][1]["n"] // 2)
    fan = h["lv"][1]["fan"]
    P0 = NP.ml_prolong_blocks(0, h["lv"][0]["geo"])
    for k in range(6):
        x = np.zeros((n, 6))
        c = np.arange(A * fan, min(n, (A + 1) * fan))
        x[c] = P0[c][:, :, k]
        xs.append(x)
    live = h["b2v"] >= 0
    for x in xs:
        x[~live] = 0.0                                                   # (an EMPTY row carries no residual)
        z = p.apply(1, x, h["lam"])
        _judge([HC.check_apply(h, x, z)], case)


def run_case(capi, n_nodes, n_edges, seed, cfg, want, case, additive=False, after=0, lam_factors=(None, 1e3), apply=True, cfg_extra=None):
    g = synth.make_pose_graph(n_nodes, n_edges, seed=seed)
    p = capi.DiagPgo(**dict(cfg, **(cfg_extra or {})))
    try:
        if additive:
            p.ban_mult()
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        for phase in range(2 if after else 1):
            if phase:
                st = p.optimize(after)
                assert st["status"] == 0
            lin = p.linearize()
            tag = "%s%s" % (case, " after optimize(%d)" % after if phase else "")
            for lf in lam_factors:
                lam = -1.0 if lf is None else lf * lin["diagmax"]
                h = check_setup(p, lin, lam, tag, want)
                if apply:
                    check_application(p, h, lam, tag)
        return h
    finally:
        p.close()


NO_SCHUR = dict(schur_reduce=-1)


# ------------------------------------------------------------------------------------------------------------------ one coarse level
def test_eight_rows_stay_block_jacobi(capi):
    g = synth.make_pose_graph(9, 20, seed=8)
    p = capi.DiagPgo(**NO_SCHUR)
    try:
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        h = p.hierarchy()
        assert h["levels"] == 0 and p.apply_info()["op"] == 0
    finally:
        p.close()


@pytest.mark.parametrize("nb", [9, 59, 64])
def test_one_coarse_level_no_dense_operator(capi, nb):
    run_case(capi, nb + 1, 3 * (nb + 1), nb, NO_SCHUR, dict(levels=1, cl=0, agg=1, mult=0, n=[nb, -(-nb // 8)]), "one level nb=%d" % nb,
             after=5 if nb == 59 else 0)


# ------------------------------------------------------------------------------------------------------------------ agg = 1, dense level 1
@pytest.mark.parametrize("nb,e", DENSE1)
def test_dense_level1_multiplicative(capi, nb, e):
    n = _levels1(nb)
    h = run_case(capi, nb + 1, e, 2 if nb == 999 else nb, NO_SCHUR, dict(levels=len(n) - 1, cl=1, agg=1, mult=1, ns_steps=2, sibling0=1, n=n),
                 "dense-1 mult nb=%d" % nb, after=5 if nb == 999 else 0)
    if nb == 1024:
        assert h["lv"][-1]["n"] == 16
    if nb == 1025:
        assert h["levels"] == 3 and h["lv"][2]["n"] == 17


@pytest.mark.parametrize("nb", range(201, 208))
def test_dense_level1_last_short_aggregate(capi, nb):
    """nb mod 8 = 1 .. 7: the last aggregate of level 1 has that many children."""
    assert nb % 8 == nb - 200
    run_case(capi, nb + 1, 3 * nb, nb, NO_SCHUR, dict(levels=2, cl=1, agg=1, mult=1, n=[nb, 26, 4]), "short aggregate nb=%d" % nb)


@pytest.mark.parametrize("nb,e", DENSE1 + [(nb, 3 * nb) for nb in range(201, 208)])
def test_dense_level1_additive_fallback(capi, nb, e):
    """The additive dense operator: what a handle applies once the multiplicative one has broken down on one of its graphs.  The same
    sizes as the multiplicative one, the last short aggregate of 1 .. 7 children included."""
    n = _levels1(nb)
    run_case(capi, nb + 1, e, 2 if nb == 999 else nb, NO_SCHUR, dict(levels=len(n) - 1, cl=1, agg=1, mult=0, ns_steps=0, n=n),
             "dense-1 additive nb=%d" % nb, additive=True, after=5 if nb == 513 else 0)


# ------------------------------------------------------------------------------------------------------------------ agg = 4, dense level 2
@pytest.mark.parametrize("nodes,e,steps,cfg", [(3074, 12300, 4, NO_SCHUR), (4000, 16000, 4, NO_SCHUR), (5000, 5600, 2, NO_SCHUR)])
def test_dense_level2(capi, nodes, e, steps, cfg):
    n = _levels4(nodes - 1)
    run_case(capi, nodes, e, {3074: 3073, 4000: 40, 5000: 50}[nodes], cfg,
             dict(levels=len(n) - 1, cl=2, agg=4, mult=1, ns_steps=2, structure_ns_steps=steps, sibling0=0, n=n), "dense-2 %d/%d" % (nodes, e),
             after=5 if nodes == 4000 else 0)


def test_dense_level2_four_newton_schulz_steps(capi):
    """4000 / 16000 asks for 4 steps at the composite level (loopy, agg = 4); the first two LM iterations take 2 (ml_ns_steps_at), every
    later one 4: those four, from the device's own X_0, with the last GEMM's f32 epilogue."""
    g = synth.make_pose_graph(4000, 16000, seed=40)
    p = capi.DiagPgo(**NO_SCHUR)
    try:
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        lin = p.linearize()
        for lf in (None, 1e3):
            lam = -1.0 if lf is None else lf * lin["diagmax"]
            h4 = p.hierarchy(lam, 4)
            assert h4["structure_ns_steps"] == 4 and h4["ns_steps"] == 4 and h4["cl"] == 2 and h4["mult"] == 1, h4["ns_steps"]
            h0 = p.hierarchy(lam, 0)
            found = HC.check_dense(h4, h0)
            assert [f.stage for f in found].count("Newton-Schulz") == 1
            _judge([f._replace(stage=f.stage + " (4 steps)") if f.stage == "Newton-Schulz" else f for f in found], "dense-2 4000/16000, 4 steps")
            HC.check_cmat32(h4)
    finally:
        p.close()


def test_dense_level2_additive_fallback(capi):
    n = _levels4(3999)
    run_case(capi, 4000, 16000, 40, NO_SCHUR, dict(levels=len(n) - 1, cl=2, agg=4, mult=0, ns_steps=0, n=n), "dense-2 additive 4000/16000",
             additive=True, after=5)


@pytest.mark.parametrize("nodes,e", [(10000, 50000), (14000, 60000)])
def test_dense_level2_per_level_geometry(capi, nodes, e):
    """C4 and a 14k / 60k graph: more than kGeoAllMax = 1024 level-1 aggregates (the per-level geometry launches); from ~12k vertices the
    ml_alpha variant of the iteration."""
    n = _levels4(nodes - 1)
    assert n[1] > 1024
    run_case(capi, nodes, e, 4, NO_SCHUR, dict(levels=len(n) - 1, cl=2, agg=4, mult=1, ns_steps=2, structure_ns_steps=4, n=n),
             "dense-2 %d/%d" % (nodes, e))


# ------------------------------------------------------------------------------------------------------------------ walked hierarchy
def test_walked_hierarchy_in_a_child_process(capi):
    """C4 under UZL_ML_NO_COMP4=1 (read once per process): agg = 4 and no dense operator - the PCG kernels walk the levels in LDS.
    Both lambdas, the poses after optimize(5), and the steady-state iteration of that variant (kCgPlain4)."""
    env = dict(os.environ, UZL_ML_NO_COMP4="1")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_hierarchy_worker.py")
    r = subprocess.run([sys.executable, worker, "walked"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["cl"] == 0 and out["agg"] == 4 and out["levels"] >= 3 and out["cg_variant"] == CG_PLAIN4, {k: v for k, v in out.items() if k != "measured"}
    assert any(k.startswith("steady state: z") for k in out["measured"])
    for k, (v, where) in out["measured"].items():
        _note(k + " (walked)", v, where)


# ------------------------------------------------------------------------------------------------------------------ Schur-reduced systems
@pytest.mark.parametrize("numbering", [1, 2])
def test_reduced_system_1500_1530(capi, numbering):
    """Row order and strong aggregates as one level: the hierarchy over the reduced matrix (its rows' poses: the separators')."""
    g = synth.make_pose_graph(1500, 1530, seed=15)
    p = capi.DiagPgo(reduced_numbering=numbering)
    try:
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        for lf in (None, 1e3, "after optimize(5)"):
            if lf == "after optimize(5)":
                assert p.optimize(5)["status"] == 0
                lf = None
            lin = p.linearize()
            lam = -1.0 if lf is None else lf * lin["diagmax"]
            h = check_setup(p, lin, lam, "Schur 1500/1530 numbering=%d" % numbering, dict(reduced=1, strong=numbering - 1, strong_blocks=0, agg=1))
            red = p.reduced(h["lam"])
            assert np.array_equal(red["row_ptr"], h["lv"][0]["row_ptr"]) and np.array_equal(red["blk"], h["lv"][0]["blk"])
            assert np.array_equal(red["hdiag"], h["lv"][0]["G"])
            if numbering == 2:
                assert (h["b2v"] < 0).any(), "the strong numbering has no EMPTY rows here"
            check_application(p, h, lam, "Schur 1500/1530 numbering=%d" % numbering)
    finally:
        p.close()


STRONG_BLOCKS = (20000, 21000, 20)                 # 3392 reduced rows in 106 blocks of 4 x 8


def test_reduced_system_strong_blocks_with_empty_rows(capi):
    """More than 256 strong groups: blocks of 4 x 8 rows padded with EMPTY rows, the agg = 4 geometry."""
    g = synth.make_pose_graph(STRONG_BLOCKS[0], STRONG_BLOCKS[1], seed=STRONG_BLOCKS[2])
    p = capi.DiagPgo(reduced_numbering=2)
    try:
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        for lf in (None, 1e3, "after optimize(5)"):
            if lf == "after optimize(5)":
                assert p.optimize(5)["status"] == 0
                lf = None
            lin = p.linearize()
            lam = -1.0 if lf is None else lf * lin["diagmax"]
            h = check_setup(p, lin, lam, "Schur strong blocks", dict(reduced=1, strong=1, strong_blocks=1, agg=4, cl=2))
            assert (h["b2v"] < 0).any()
            check_application(p, h, lam, "Schur strong blocks")
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------------------------ the fused iteration
CG_PLAIN1, CG_COMP1, CG_PLAIN4, CG_COMP4, CG_COMP4_YPRE, CG_COMP4_VPRE = range(6)       # pgo_types.hpp: LmCgVariant
# ml_cg_variant: no dense operator - plain1 / plain4 (the walked hierarchy: _hierarchy_worker.py); dense level 1 - comp1; dense level 2 -
# Ypre while 6 n_2 <= 2304 (4000 / 16000, C4), the ml_alpha variant Vpre above (14k / 60k).  kCgComp4 itself is what a hierarchy without
# a Vg buffer would take: upload_ml always gives one, so no graph reaches it.
STEADY = {"59 one level": (60, 180, 59, {}, dict(cl=0, agg=1, cg_variant=CG_PLAIN1)),
          "513": (514, 2000, 513, {}, dict(cl=1, agg=1, cg_variant=CG_COMP1)), "C2": (1000, 5000, 2, {}, dict(cl=1, agg=1, cg_variant=CG_COMP1)),
          "4000/16000": (4000, 16000, 40, {}, dict(cl=2, agg=4, cg_variant=CG_COMP4_YPRE)),
          "C4": (10000, 50000, 4, {}, dict(cl=2, agg=4, cg_variant=CG_COMP4_YPRE)),
          "14000/60000": (14000, 60000, 4, {}, dict(cl=2, agg=4, cg_variant=CG_COMP4_VPRE)),
          "1500/1530 reduced": (1500, 1530, 15, None, dict(cl=1, agg=1, reduced=1, cg_variant=CG_COMP1))}


def run_steady(capi, nodes, e, seed, cfg, want, case):
    g = synth.make_pose_graph(nodes, e, seed=seed)
    p = capi.DiagPgo(pcg_stop=1, pcg_tol=1e-14, **(NO_SCHUR if cfg is not None else {}))
    try:
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        lin = p.linearize()
        h = p.hierarchy()
        for key, v in want.items():
            assert h[key] == v, "%s is not the class it claims: %s = %s" % (case, key, h[key])
        red = p.reduced(h["lam"])
        b = lin["b"] if red is None else red["b"]
        assert (red is not None) == bool(h["reduced"]) and b.shape[0] == h["rows"]
        st = {}
        for k in (0, 1, 2, 3, 5, 6, 7):
            st[k] = p.pcg_state(k, h["lam"])
            assert st[k]["done"] == 0 and st[k]["lam"] == h["lam"], (k, st[k]["done"], st[k]["its"])
        for k in (1, 2, 3, 7):
            assert np.abs(st[k]["x"]).max() > 0
            _judge(HC.check_steady_state(h, st[k], b, k) + [HC.check_direction(st.get(k - 2), st[k - 1], st[k])], "%s k=%d" % (case, k))
        return h
    finally:
        p.close()


@pytest.mark.parametrize("case", sorted(STEADY))
def test_steady_state_iteration(capi, case):
    """After k = 1, 2, 3, 7 PCG iterations (uzl_debug_pgo_pcg_state; pcg_tol out of reach, so no iteration is a no-op): the gather-level
    residual the next ml_cg would read is P^T r of the dumped r, z = M^-1 r (hierarchy_checks.check_steady_state), and the direction
    the iteration formed is z + beta p_old of the two states before (check_direction).  Every case asserts its ml_cg variant."""
    run_steady(capi, *STEADY[case], case)


# ------------------------------------------------------------------------------------------------------------------ PCG iteration counts
def _k_progress_every():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uzliti_slam_amd", "csrc", "pgo_types.hpp")).read()
    return int(re.search(r"constexpr int kProgressEvery = (\d+);", src).group(1))


K_PROGRESS_EVERY = _k_progress_every()                   # pgo_types.hpp
ITERATIONS = {"513": (514, 2000, 513, NO_SCHUR), "C2": (1000, 5000, 2, NO_SCHUR), "4000/16000": (4000, 16000, 40, NO_SCHUR),
              "1500/1530 reduced": (1500, 1530, 15, {})}


@pytest.mark.parametrize("case", sorted(ITERATIONS))
def test_pcg_iteration_count_is_the_reference_operators(capi, case):
    """cfg.pcg_stop = 1, pcg_tol = 1e-7: the device's PCG iteration count against a float64 NumPy PCG on the same system (the level-0 arrays
    the device holds) with the float64 REFERENCE operator built from that system and the rows' poses (hierarchy_checks.
    reference_hierarchy, Y_cl rounded to f32 as the device applies it).  A preconditioner that is subtly wrong converges, more slowly:
    this is where that shows as a number.  Margin: the stop test's look interval - the relative test of pcg_stop = 1 is taken by every
    ml_spmv, i.e. every iteration; kProgressEvery = 2 covers it - plus the spread the reference alone shows between the f32-rounded and
    the unrounded Y_cl - 0 on all four systems (measured on the CPU; the counts are in the module docstring), so the margin is 2."""
    nodes, e, seed, cfg = ITERATIONS[case]
    g = synth.make_pose_graph(nodes, e, seed=seed)
    tol = 1e-7
    p = capi.DiagPgo(pcg_stop=1, pcg_tol=tol, **cfg)
    try:
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
        lin = p.linearize()
        h = p.hierarchy()
        out = p.solve(h["lam"])
        assert out["converged"] and out["guard_trips"] == 0 and out["lam"] == h["lam"], out
        red = p.reduced(h["lam"])
        b = lin["b"] if red is None else red["b"]
        lv0 = h["lv"][0]
        t, R = rows_poses(h, lin)
        ref, _ = HC.reference_hierarchy(lv0["row_ptr"], lv0["col"], lv0["blk"], lv0["G"], t, R, h["lam"], agg=h["agg"], cl=h["cl"], mult=h["mult"],
                                        ns_steps=h["ns_steps"], upper_ns=h["upper_ns"], sibling0=h["sibling0"], fans=HC.fans_of(h))
        assert [lv["n"] for lv in ref["lv"]] == [lv["n"] for lv in h["lv"]]
        A = NP.bcsr_to_sparse(lv0["row_ptr"], lv0["col"], lv0["blk"], diag=lv0["G"] + h["lam"] * np.eye(6), nrows=lv0["n"])
        its32, _ = HC.reference_pcg(A, b, lambda r: HC.apply_reference(ref, r), tol)
        n6 = 6 * ref["lv"][ref["cl"]]["n"]
        exact = dict(ref, Cmat32=ref["lv"][ref["cl"]]["Y"][:, :n6])
        its64, _ = HC.reference_pcg(A, b, lambda r: HC.apply_reference(exact, r), tol)
        print("\nPCG iterations %s: device %d, reference (f32 Y_cl) %d, reference (f64 Y_cl) %d" % (case, out["its"], its32, its64))
        _note("PCG iterations %s: |device - reference|" % case, abs(out["its"] - its32), "device %d, reference %d / %d" % (out["its"], its32, its64))
        assert abs(out["its"] - its32) <= K_PROGRESS_EVERY + abs(its32 - its64), (out["its"], its32, its64)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------------------------ second hierarchy copy
def test_hook_after_an_optimize_that_rebuilt_ahead(capi):
    """C2: optimize rebuilds the second hierarchy copy ahead on the second stream; the hook on the same handle afterwards still returns a
    hierarchy that agrees, stage by stage, with the reference at the CURRENT poses - and leaves the handle as usable as it found it."""
    g = synth.make_pose_graph(1000, 5000, seed=2)
    res = []
    for hooks in (False, True):
        p = capi.DiagPgo()
        try:
            p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
            st = p.optimize(4)
            assert st["status"] == 0 and st["precond_builds"] >= 2, st
            if hooks:
                lin = p.linearize()
                assert not np.array_equal(lin["poses"], np.asarray(g["nodes_pose"]).reshape(-1, 12))
                h = check_setup(p, lin, -1.0, "C2 after optimize(4)", dict(cl=1, agg=1, mult=1))
                check_application(p, h, -1.0, "C2 after optimize(4)")
            st = p.optimize(4)
            res.append((p.store()[0], st["chi2_final"], st["lm_trials"]))
        finally:
            p.close()
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1:] == res[1][1:]
