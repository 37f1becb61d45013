"""The pose-graph linear system stage by stage against a float64 reference (uzl_debug_pgo_linearize / uzl_debug_pgo_solve of the
diagnostic library, capi.DiagPgo).

The end-to-end tests (test_pgo_gpu.py) pin the error function and the gradient b: the LM fixed point depends on nothing else, and a
wrong Hessian block, SpMV slot, Schur term or preconditioner only slows LM down.  These tests look at H and at one linear solve.

Reference: np_reference.build_system on the oracle-flattened graph (skip rules, xy-only, sensors from the oracle) with the oracle's
analytic Jacobians, at the very poses the hook linearised at.

Tolerances (round-off bounds, never "close enough for the pose bar"):
  * H, per entry:  |H - H_ref| <= C_H eps S_H,  S_H = sum over the edges of (|J_a| + s)^T |Omega'| (|J_c| + s) (np_reference.system_magnitudes;
    s as below: a Jacobian entry is a product of rotations and relative translations, known to a few eps s absolutely).  Every entry
    of a block that an edge forms has S_H >= s^2 min diag(Omega') > 0, so no floor is needed; S_H = 0 where no edge joins two free vertices,
    and any nonzero value there fails;
  * b, per entry:  |b - b_ref| <= C_H eps S_b,  S_b = sum (|J_a| + s)^T |Omega'| (|e| + s): an edge error is a difference of translations of
    size s = 1 + |t_i| + |t_j| + |t_z|, known only to eps s absolutely - at the LM fixed point, where b is itself rounding noise, the bound
    is absolute per term;
  * chi2:  C_H eps sum (|e| + s)^T |Omega| (|e| + s).
  C_H = 1e3.  A dropped or duplicated slot is an error of the size of a whole block, i.e. of the order of S_H itself: ~1e12 times the
  bound (a block's H_aa share dropped per 256-slot chunk fails at 4.5e12 in the CPU dry run of this check).

The solve (uzl_debug_pgo_solve) against scipy's sparse direct solve of (H_ref + lambda I) dx = b_ref, all vertices (Schur interiors
included), checks include/uzl_mi355x.h's promise for cfg.pcg_stop = 0: error of dx below pcg_tol in every translation component and
below 0.1 pcg_tol in every quaternion-vector component.  For pcg_stop = 1 the relative test r.M^-1 r <= pcg_tol^2 r0.M^-1 r0 is checked
on the recurrence's own numbers.  Every solve must report converged with no residual-guard trip.

Measured on an MI355X (pytest -s prints the MEASURED table at the end of the module):
  * H / b / chi2 against their bounds, worst over every graph above: 3.6e-3 / 6.5e-5 / 3.1e-7 (H: C2 after optimize(20)).
  * dx error relative to the promise, max(err_t / pcg_tol, err_q / (0.1 pcg_tol)), worst per path at lambda_init (pcg_tol 1e-5 | 1e-7):
        block-Jacobi (300 / 1200)                   0.44 | 0.095
        multilevel AGG = 1, dense level 1 (65)      0.054 | 0.053
                                  (513)             0.22 | 0.43
                                  (1281)            0.46 | 0.45
        multilevel AGG = 4, dense level 2 (4000)    0.55 | 0.37
        Schur, row order (1500 / 1530)              0.45 | 0.12
        Schur, strong aggregates (1500 / 1530)      0.24 | 0.11
        everything eliminated                       7e-9
        long chain, one far closure (4000)          0.12 | 0.69;  not Schur-reduced 0.23
        C4 (10k / 50k)                              0.48
    At lambda = 1e3 max diag every path is below 1e-4.  The promise holds everywhere it was tested, with a margin of 1.4x at worst.
  * pcg_stop = 1, pcg_tol 1e-7: the largest error seen was 0.96 pcg_tol (multilevel, 1281 vertices).  The relative test does not
    promise a step error, so only its own stop condition is asserted.
  * Recurrence residual against |b - A dx| (check_recurrence_residual): at most 0.023 of the drift bound (long chain, not reduced, large lambda).
  * SpMV (b), op 0 against its bound: 1.4e-3 .. 2.0e-3 on every graph (worst: the hub's long rows); reduced SpMV 2.0e-3.
  * Schur complement (c), 600 / 630 chain, both numberings: matrix 5.2e-4, right-hand side 2.1e-5 of the bound.
  * Preconditioner (d): block-Jacobi inverse 4.5e-4 of its bound; additive operator symmetric to 3.1e-8 of its bound;
    kappa(M^-1 A) at lambda_init = 15.94 (additive, 59 free vertices) and 19.25 (multiplicative, C1).  Both are asserted at 2x.
    The float64 reference application of the same hierarchies (hierarchy_checks.apply_reference) has kappa 15.9379 and 19.253; the
    device's extreme eigenvalues are within 2.3e-6 / 1.7e-6 of the derived margin | |dM| |A| |_2 (1.6e-9 / 3.9e-9) of the reference's.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import np_reference as NP
from uzliti_slam_amd import synth

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
C_H = 1e3

MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nMEASURED (stage / worst ratio to its bound):")
        for k in sorted(MEASURED):
            print("  %-60s %.3e" % (k, MEASURED[k]))


def _note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(v))


# ------------------------------------------------------------------------------------------------------------------ graphs
def _edges(frm, to, Z, info=400.0):
    E = len(frm)
    I12 = np.eye(3, 4).reshape(12)
    return {"from": np.asarray(frm, np.int32), "to": np.asarray(to, np.int32), "type": np.full(E, synth.EDGE_TYPE_3D_FULL, np.int32),
            "sensor_from": np.full(E, -1, np.int32), "sensor_to": np.full(E, -1, np.int32), "valid": np.ones(E, np.int32),
            "transform": np.asarray(Z).reshape(E, 12), "displacement_from": np.tile(I12, (E, 1)), "displacement_to": np.tile(I12, (E, 1)),
            "information": np.tile((np.eye(6) * info).reshape(36), (E, 1)), "diff_time": np.zeros(E)}


def _concat_edges(a, b):
    return {k: np.concatenate([np.asarray(a[k]), np.asarray(b[k])]) for k in a}


def _measure(gt, frm, to, rng, sig_t=0.01, sig_r=0.002):
    Z = synth.se3_mul(synth.se3_inv(gt[frm]), gt[to])
    return synth.se3_mul(Z, synth.se3_from_noise(rng.normal(0, sig_t, (len(frm), 3)), rng.normal(0, sig_r, (len(frm), 3))))


def hub_graph():
    """A 400-vertex graph whose vertex 7 carries 330 slots (past one 256-slot chunk of the Hessian build), 30 of them repeated
    multi-edges (the same pair several times: several slots of one block)."""
    rng = np.random.default_rng(11)
    g = synth.make_pose_graph(400, 800, seed=21, outlier_frac=0.0)
    gt = g["gt_pose"].reshape(-1, 3, 4)
    others = rng.choice(np.setdiff1d(np.arange(400), [7]), 300, replace=False)
    others = np.concatenate([others, others[:10], others[:10], others[5:15]])
    frm = np.full(len(others), 7); to = others
    g["edges"] = _concat_edges(g["edges"], _edges(frm, to, _measure(gt, frm, to, rng)))
    return g


def middle_fixed_two_components():
    """Fixed vertices in the middle of a graph, and a second component with nothing fixed (gauge-fixed by the handle)."""
    a = synth.make_pose_graph(300, 900, seed=5)
    b = synth.make_pose_graph(60, 150, seed=6)
    fixed = np.concatenate([np.asarray(a["nodes_fixed"]).copy(), np.zeros(60, np.uint8)])
    fixed[[120, 121, 250]] = 1
    eb = {k: np.array(v) for k, v in b["edges"].items()}
    eb["from"] = eb["from"] + 300; eb["to"] = eb["to"] + 300
    return dict(nodes_pose=np.concatenate([a["nodes_pose"], b["nodes_pose"]]), nodes_fixed=fixed.astype(np.uint8),
                gt_pose=np.concatenate([a["gt_pose"], b["gt_pose"]]), edges=_concat_edges(a["edges"], eb))


def sensor_graph():
    rng = np.random.default_rng(5)
    g = synth.make_pose_graph(150, 500, seed=6)
    E = len(g["edges"]["from"])

    def rand_T(k, scale):
        return synth.se3(synth.quat_to_R(synth.quat_from_rotvec(rng.normal(0, scale, (k, 3)))), rng.normal(0, scale, (k, 3)))

    sensors = rand_T(3, 0.2).reshape(-1, 12)
    g["edges"]["sensor_from"] = rng.integers(-1, 3, E).astype(np.int32)
    g["edges"]["sensor_to"] = rng.integers(-1, 3, E).astype(np.int32)
    g["edges"]["displacement_from"] = rand_T(E, 0.05).reshape(-1, 12)
    g["edges"]["displacement_to"] = rand_T(E, 0.05).reshape(-1, 12)
    return g, sensors


def huber_graph():
    """20 % outliers and initial poses far from the solution: many Huber-active edges."""
    rng = np.random.default_rng(9)
    g = synth.make_pose_graph(300, 1200, seed=3, outlier_frac=0.2)
    P = np.asarray(g["nodes_pose"]).reshape(-1, 3, 4).copy()
    P[1:] = synth.se3_mul(P[1:], synth.se3_from_noise(rng.normal(0, 0.5, (len(P) - 1, 3)), rng.normal(0, 0.2, (len(P) - 1, 3))))
    g["nodes_pose"] = P.reshape(-1, 12)
    return g


def long_chain_one_closure():
    """test_pgo_gpu.py::test_ill_conditioned_long_chain_one_far_closure's graph: 4000-vertex chain, one loop closure 3 -> 3990."""
    g = synth.make_pose_graph(4000, 4000, seed=31, outlier_frac=0.0)
    e = {k: np.asarray(v).copy() for k, v in g["edges"].items()}
    gt = g["gt_pose"].reshape(-1, 3, 4)
    k = len(e["from"]) - 1
    e["from"][k] = 3; e["to"][k] = 3990
    e["transform"][k] = synth.se3_mul(synth.se3_inv(gt[3:4]), gt[3990:3991]).reshape(12)
    g["edges"] = e
    return g


def everything_eliminated():
    """test_schur_gpu.py::test_everything_eliminated's graph: chains hanging off the fixed vertex, no separator left."""
    rng = np.random.default_rng(2)
    arms, L = 5, 20
    n = 1 + arms * L
    gt = np.tile(np.eye(3, 4), (n, 1, 1))
    frm, to = [], []
    for a in range(arms):
        prev = 0
        for k in range(L):
            v = 1 + a * L + k
            step = synth.se3_from_noise(np.array([[0.3, 0.02 * a, 0.0]]), np.array([[0.0, 0.0, 0.1 * (a - 2)]]))[0]
            gt[v] = synth.se3_mul(gt[prev], step)
            frm.append(prev); to.append(v); prev = v
    frm = np.array(frm); to = np.array(to)
    Z = _measure(gt, frm, to, rng)
    init = gt.copy()
    init[1:] = synth.se3_mul(gt[1:], synth.se3_from_noise(rng.normal(0, 0.05, (n - 1, 3)), rng.normal(0, 0.02, (n - 1, 3))))
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    return dict(nodes_pose=init.reshape(n, 12), nodes_fixed=fixed, gt_pose=gt.reshape(n, 12), edges=_edges(frm, to, Z))


# ------------------------------------------------------------------------------------------------------------------ reference
class System:
    """The reference system at the poses the handle linearised at, in the handle's row numbering."""

    def __init__(self, oracle, g, lin, xy=False, sensors=None, use_odometry_parameters=False, extra=None):
        """extra [input edges]: a magnitude added to s of every edge (np_reference.system_magnitudes), e.g. the translation norms of the
        sensor and displacement factors its measurement was composed from."""
        fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"], sensors=sensors, optimize_xy_only=xy,
                                  use_odometry_parameters=use_odometry_parameters)
        extra = None if extra is None else np.asarray(extra, np.float64)[fl["src_edge"]]
        fixed, _ = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
        X = lin["poses"].reshape(-1, 3, 4)
        ij, Z = fl["ij"], fl["meas"].reshape(-1, 3, 4)
        J = [oracle.edge_jacobians(X[i], X[j], Z[k]) for k, (i, j) in enumerate(ij)]
        jac = (np.array([a for a, _ in J]).reshape(-1, 6, 6), np.array([b for _, b in J]).reshape(-1, 6, 6))
        H, b, chi = NP.build_system(lin["poses"], fixed, ij, fl["meas"], fl["info"], fl["robust"], jac=jac)
        Hm, bm = NP.system_magnitudes(lin["poses"], fixed, ij, fl["meas"], fl["info"], fl["robust"], jac, extra=extra)
        e = NP.edge_errors(lin["poses"], ij, fl["meas"])
        P = X
        s = 1.0 + np.abs(P[ij[:, 0], :, 3]).max(1) + np.abs(P[ij[:, 1], :, 3]).max(1) + np.abs(Z[:, :, 3]).max(1)
        if extra is not None:
            s = s + extra
        self.fl, self.e, self.s = fl, e, s
        ae = np.abs(e) + s[:, None]
        self.chi_mag = float(np.einsum("ki,kij,kj->", ae, np.abs(fl["info"]).reshape(-1, 6, 6), ae))
        v2b = lin["v2b"]
        assert np.array_equal(v2b < 0, fixed != 0), "the handle's free vertices are not the oracle's"
        nb = int((v2b >= 0).sum())
        b2v = np.empty(nb, np.int64); b2v[v2b[v2b >= 0]] = np.nonzero(v2b >= 0)[0]
        idx = NP.block_index(b2v)
        self.n, self.nb, self.b2v, self.v2b = len(v2b), nb, b2v, v2b
        self.H = H[idx][:, idx].tocsr(); self.Hm = Hm[idx][:, idx].tocsr()
        self.b = b[idx]; self.bm = bm[idx]; self.chi = chi

    def to_vertices(self, x):
        out = np.zeros((self.n, 6))
        out[self.b2v] = np.asarray(x).reshape(-1, 6)
        return out


def check_linearization(lin, R, key):
    """(a): every H_ac (slots summed per block), H_aa, b, chi2; H_ac = H_ca^T; no block where no edge joins two free vertices."""
    Hg = NP.bcsr_to_sparse(lin["row_ptr"], lin["col"], lin["blk"], diag=lin["haa"], nrows=R.nb)
    Hm = R.Hm
    D = abs(Hg - R.H).tocoo()
    tol = C_H * EPS * np.asarray(Hm[D.row, D.col]).reshape(-1)      # (0 where no edge joins the two vertices: any value there fails)
    worst = (D.data / tol).max() if D.nnz else 0.0
    _note(key + " H / bound", worst)
    assert worst <= 1.0, "H differs from the reference by %.3g x the round-off bound at (%d, %d)" % (
        worst, D.row[np.argmax(D.data / tol)], D.col[np.argmax(D.data / tol)])
    T = abs(Hg - Hg.T).tocoo()
    if T.nnz:
        tt = 2 * C_H * EPS * np.asarray(Hm[T.row, T.col]).reshape(-1)
        assert (T.data <= tt).all(), "H_ac and H_ca are not transposes of each other"
    db = np.abs(lin["b"].reshape(-1) - R.b)
    wb = (db / (C_H * EPS * R.bm)).max() if R.nb else 0.0
    _note(key + " b / bound", wb)
    assert wb <= 1.0, "b differs from the reference by %.3g x the round-off bound" % wb
    wc = abs(lin["chi2"] - R.chi) / (C_H * EPS * R.chi_mag)
    _note(key + " chi2 / bound", wc)
    assert wc <= 1.0, (lin["chi2"], R.chi)


def _linearize_case(capi, oracle, g, key, cfg=None, sensors=None, after=0, extra=None):
    xy = bool((cfg or {}).get("optimize_xy_only", 0))
    kw = dict(use_odometry_parameters=bool((cfg or {}).get("use_odometry_parameters", 0)), extra=extra)
    p = capi.DiagPgo(**(cfg or {}))
    try:
        p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"], sensors=sensors)
        lin = p.linearize()
        check_linearization(lin, System(oracle, g, lin, xy, sensors, **kw), key + " initial")
        if after:
            st = p.optimize(after)
            assert st["status"] == 0
            lin = p.linearize()
            check_linearization(lin, System(oracle, g, lin, xy, sensors, **kw), key + " after optimize(%d)" % after)
        return lin
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------------------------ (a) Hessian
def test_hessian_c1_and_c2(capi, oracle):
    _linearize_case(capi, oracle, synth.make_pose_graph(100, 300), "C1", after=20)
    _linearize_case(capi, oracle, synth.make_pose_graph(1000, 5000, seed=2), "C2", after=20)


def test_hessian_hub_row_past_one_chunk_with_multi_edges(capi, oracle):
    lin = _linearize_case(capi, oracle, hub_graph(), "hub", after=5)
    assert np.diff(lin["row_ptr"]).max() > 256           # the case is what it says: one row spans more than one chunk


@pytest.mark.parametrize("nb", [41, 42, 43, 84, 85])
def test_hessian_rows_at_workgroup_boundaries(capi, oracle, nb):
    lin = _linearize_case(capi, oracle, synth.make_pose_graph(nb + 1, 3 * (nb + 1), seed=nb), "nb=%d" % nb)
    assert len(lin["row_ptr"]) - 1 == nb


def test_hessian_fixed_in_the_middle_and_gauge_fixed_component(capi, oracle):
    lin = _linearize_case(capi, oracle, middle_fixed_two_components(), "fixed+components", after=5)
    assert (lin["col"] == -1).any()                       # slots whose neighbour is fixed exist


def test_hessian_permuted_vertex_order(capi, oracle):
    g = synth.make_pose_graph(300, 900, seed=8)
    perm = np.random.default_rng(4).permutation(300)
    lin = _linearize_case(capi, oracle, synth.permute_graph(g, perm), "permuted")
    free = lin["v2b"] >= 0
    assert not np.array_equal(lin["v2b"][free], np.arange(free.sum()))


def test_hessian_xy_only_and_sensors(capi, oracle):
    _linearize_case(capi, oracle, synth.make_pose_graph(200, 600, seed=12), "xy-only", cfg=dict(optimize_xy_only=1), after=5)
    g, sensors = sensor_graph()
    _linearize_case(capi, oracle, g, "sensors", sensors=sensors, after=5)


def test_hessian_many_huber_active_edges(capi, oracle):
    _linearize_case(capi, oracle, huber_graph(), "huber", after=20)


def test_hessian_c4_sparse(capi, oracle):
    _linearize_case(capi, oracle, synth.make_pose_graph(10000, 50000, seed=4), "C4")


# ------------------------------------------------------------------------------------------------------------------ (e) one solve
def check_solve(p, oracle, g, key, lam_factor=None):
    """One solve at lambda_init (lam_factor None) or lam_factor * max diag, against spsolve of the reference system."""
    lin = p.linearize()
    R = System(oracle, g, lin)
    lam = -1.0 if lam_factor is None else lam_factor * lin["diagmax"]
    out = p.solve(lam)
    lam = out["lam"]
    A = (R.H + lam * sp.identity(6 * R.nb, format="csr")).tocsc()
    x_ref = spl.splu(A).solve(R.b)
    dx_ref = R.to_vertices(x_ref)
    assert out["converged"] and out["guard_trips"] == 0, out
    tol, stop = p.cfg.pcg_tol, p.cfg.pcg_stop
    et, eq = NP.step_error(out["dx"], dx_ref)
    assert np.all(out["dx"][R.v2b < 0] == 0)
    if stop == 0:
        w = max(et / tol, eq / (0.1 * tol))
        _note("%s dx error / pcg_tol promise" % key, w)
        assert et <= tol and eq <= 0.1 * tol, "step error %.3g m / %.3g (q) at pcg_tol %.0e" % (et, eq, tol)
    else:
        assert out["rz_end"] <= out["rz_stop"], out
        _note("%s (pcg_stop=1) dx error / pcg_tol" % key, max(et, eq) / tol)
    if lam_factor is not None and lam_factor >= 1e2:
        # dx = (I + H / lam)^-1 b / lam, so |dx - b / lam|_inf <= q / (1 - q) |b|_inf / lam with q = |H|_inf / lam (the largest absolute
        # row sum), plus the solve's own error
        q = abs(R.H).sum(axis=1).max() / lam
        assert q < 0.5
        err = np.abs(out["dx"] - R.to_vertices(R.b) / lam).max()
        assert err <= q / (1 - q) * np.abs(R.b).max() / lam + max(tol, et, eq), (err, q)
    check_recurrence_residual(p, R, out, lam, key)
    return out


def check_recurrence_residual(p, R, out, lam, key):
    """The recurrence residual the PCG ends with (|r|^2 / |b|^2, what residual_guard reads) against the true residual b - A dx of the
    system it iterated on (the reduced one when the structure has a reduction: its matrix as the reduction hook returns it, checked in
    (c)).  Drift bound: every PCG iteration updates x += alpha p and r -= alpha A p with one rounding each, and forms A p with one more;
    the gap r - (b - A x) grows by at most C_R eps (|A| |x| + |b|) per iteration in norm (C_R = 1e3 covers the row sums of up to a few
    hundred terms), so | |r| - |b - A dx| | <= C_R eps (its + 1) ( | |A| |dx| | + |b| )."""
    red = p.reduced(lam)
    if red is None:
        A = R.H + lam * sp.identity(6 * R.nb, format="csr")
        b = R.b
        x = out["dx"][R.b2v].reshape(-1)
        Aabs = abs(R.H) + lam * sp.identity(6 * R.nb, format="csr")
    else:
        live = red["sep_rows"] >= 0
        hd = red["hdiag"].copy(); hd[live] += lam * np.eye(6)
        A = NP.bcsr_to_sparse(red["row_ptr"], red["col"], red["blk"], diag=hd, nrows=len(hd))
        Aabs = abs(A)
        b = red["b"].reshape(-1)
        xv = np.zeros((len(hd), 6))
        xv[live] = out["dx"][R.b2v[red["sep_rows"][live]]]
        x = xv.reshape(-1)
    nb_ = np.linalg.norm(b)
    if nb_ == 0:
        return
    r_true = np.linalg.norm(b - A @ x)
    r_rec = np.sqrt(max(out["res_ratio"], 0.0)) * nb_
    drift = 1e3 * EPS * (out["its"] + 1) * (np.linalg.norm(Aabs @ np.abs(x)) + nb_)
    w = abs(r_rec - r_true) / drift
    _note("%s recurrence residual / drift bound" % key, w)
    assert w <= 1.0, "recurrence residual %.3e, true residual %.3e, drift bound %.3e" % (r_rec, r_true, drift)


def _solve_case(capi, oracle, g, key, cfgs=(dict(),), lam_factors=(None, 1e3), iterations_before=0):
    for cfg in cfgs:
        p = capi.DiagPgo(**cfg)
        try:
            p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
            if iterations_before:
                p.optimize(iterations_before)
            for lf in lam_factors:
                check_solve(p, oracle, g, "%s %s lam=%s" % (key, cfg, "init" if lf is None else "%g maxdiag" % lf), lf)
        finally:
            p.close()


def test_solve_block_jacobi(capi, oracle):
    g = synth.make_pose_graph(300, 1200, seed=13)
    _solve_case(capi, oracle, g, "block-Jacobi",
                cfgs=(dict(preconditioner=0), dict(preconditioner=0, pcg_tol=1e-7), dict(preconditioner=0, pcg_stop=1, pcg_tol=1e-7)))


@pytest.mark.parametrize("n,e", [(65, 200), (513, 2000), (1281, 5000)])
def test_solve_multilevel_dense_level1(capi, oracle, n, e):
    _solve_case(capi, oracle, synth.make_pose_graph(n, e, seed=n), "ML n=%d" % n,
                cfgs=(dict(), dict(pcg_tol=1e-7), dict(pcg_stop=1, pcg_tol=1e-7)))


def test_solve_multilevel_agg4_dense_level2(capi, oracle):
    _solve_case(capi, oracle, synth.make_pose_graph(4000, 16000, seed=40), "ML AGG=4 n=4000", cfgs=(dict(), dict(pcg_tol=1e-7)))


@pytest.mark.parametrize("numbering", [1, 2])
def test_solve_schur_reduced(capi, oracle, numbering):
    _solve_case(capi, oracle, synth.make_pose_graph(1500, 1530, seed=15), "Schur 1500/1530 numbering=%d" % numbering,
                cfgs=(dict(reduced_numbering=numbering), dict(reduced_numbering=numbering, pcg_tol=1e-7)))


def test_solve_everything_eliminated(capi, oracle):
    _solve_case(capi, oracle, everything_eliminated(), "everything eliminated")


def test_solve_long_chain_one_far_closure(capi, oracle):
    _solve_case(capi, oracle, long_chain_one_closure(), "long chain",
                cfgs=(dict(), dict(pcg_tol=1e-7), dict(pcg_stop=1, pcg_tol=1e-7), dict(schur_reduce=-1)))


def test_solve_c4(capi, oracle):
    _solve_case(capi, oracle, synth.make_pose_graph(10000, 50000, seed=4), "C4", lam_factors=(None,))


def test_hooks_leave_the_handle_usable(capi, oracle):
    """optimize after linearize + solve gives the bits of an optimize on a handle that never saw a hook."""
    g = synth.make_pose_graph(513, 2000, seed=7)
    res = []
    for hooks in (False, True):
        p = capi.DiagPgo()
        try:
            p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
            if hooks:
                p.linearize(); p.solve(); p.solve(1e-2)
            st = p.optimize(10)
            res.append((p.store()[0], st["chi2_final"], st["lm_trials"]))
        finally:
            p.close()
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1:] == res[1][1:]


# ------------------------------------------------------------------------------------------------------------------ (b) SpMV
def _system(capi, oracle, g, cfg):
    p = capi.DiagPgo(**cfg)
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    lin = p.linearize()
    return p, lin, System(oracle, g, lin)


def check_spmv(p, lin, R, key):
    """op 0 against (H_ref + lambda I) x at lambda = 0, lambda_init, 1e3 max diag: |y - y_ref| <= C_H eps ((S_H + lambda I) |x|) per
    entry (the H of the kernel is within that bound of H_ref - (a) - and the SpMV adds the products of one row in some order)."""
    rng = np.random.default_rng(R.nb)
    for lam in (0.0, 1e-5 * lin["diagmax"], 1e3 * lin["diagmax"]):
        x = rng.normal(size=(R.nb, 6))
        y = p.apply(0, x, lam).reshape(-1)
        xv = x.reshape(-1)
        y_ref = R.H @ xv + lam * xv
        tol = C_H * EPS * (R.Hm @ np.abs(xv) + lam * np.abs(xv))
        w = (np.abs(y - y_ref) / tol).max()
        _note("%s SpMV / bound" % key, w)
        assert w <= 1.0, "SpMV differs by %.3g x its bound at lambda %.3g" % (w, lam)


# (AGG = 4 starts above 3072 free vertices on graphs with >= 6 slots per row, above 4096 otherwise - ml_plan: agg1_max; 3073 is the first)
@pytest.mark.parametrize("case", ["C1", "agg4-3073", "agg4-4000", "hub-long-rows", "block-Jacobi", "nb=85"])
def test_spmv(capi, oracle, case):
    graphs = {"C1": (synth.make_pose_graph(100, 300), {}), "agg4-3073": (synth.make_pose_graph(3074, 12300, seed=3073), {}),
              "agg4-4000": (synth.make_pose_graph(4000, 16000, seed=40), {}), "hub-long-rows": (hub_graph(), {}),
              "block-Jacobi": (synth.make_pose_graph(300, 1200, seed=13), dict(preconditioner=0)),
              "nb=85": (synth.make_pose_graph(86, 258, seed=85), {})}
    g, cfg = graphs[case]
    p, lin, R = _system(capi, oracle, g, dict(cfg, schur_reduce=-1))
    try:
        info = p.apply_info()
        if case.startswith("agg4"):
            assert info["agg"] == 4, info
        if case == "C1":
            assert info["agg"] == 1, info
        if case == "hub-long-rows":
            assert np.diff(lin["row_ptr"]).max() > 20
        if case == "block-Jacobi":
            assert info["op"] == 0, info
        check_spmv(p, lin, R, case)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------------------------ (c) Schur complement
def chain_with_closures(n=600, e=630, seed=15):
    return synth.make_pose_graph(n, e, seed=seed)


def check_reduced(p, lin, R, key):
    """The reduced block-CSR, its diagonal and right-hand side against the dense Schur complement of H_ref + lambda I over the separators:
        |S - S_ref| <= C_H eps (S_ss + S_si W + W^T S_is + W^T S_ii W),  W = |A_ii^-1| |A_is|,
    with S_H (+ lambda I) in place of |A| - the componentwise bound of a block elimination (|A_ss| + |A_si| |A_ii^-1| |A_is|) with the
    kernel's H error (a) carried through it; the right-hand side likewise with S_b and |A_ii^-1| |b_i|.  Empty rows of the strong
    numbering: diagonal block exactly I, right-hand side exactly 0, no nonzero block in their row or column."""
    out = []
    for lam in (1e-5 * lin["diagmax"], 1e3 * lin["diagmax"]):
        red = p.reduced(lam)
        assert red is not None, "the structure has no Schur reduction"
        sep = red["sep_rows"]; live = sep >= 0; nr = len(sep)
        empty = np.nonzero(~live)[0]
        assert np.array_equal(red["hdiag"][empty], np.tile(np.eye(6), (len(empty), 1, 1)))
        assert np.all(red["b"][empty] == 0)
        S = NP.bcsr_to_sparse(red["row_ptr"], red["col"], red["blk"], nrows=nr).toarray()
        Ee = NP.block_index(empty)
        assert np.all(S[Ee, :] == 0) and np.all(S[:, Ee] == 0)
        hd = red["hdiag"].copy(); hd[live] += lam * np.eye(6)
        keep_blocks = sep[live]
        Li = NP.block_index(np.nonzero(live)[0])
        S = S[np.ix_(Li, Li)] + sp.block_diag(list(hd[live])).toarray()
        A = (R.H + lam * sp.identity(6 * R.nb, format="csr")).toarray()
        S_ref, g_ref = NP.schur_dense(A, R.b, keep_blocks)
        Hm = R.Hm.toarray() + lam * np.eye(6 * R.nb)
        k = NP.block_index(keep_blocks); i = NP.block_index(np.setdiff1d(np.arange(R.nb), keep_blocks))
        Ainv = np.abs(np.linalg.inv(A[np.ix_(i, i)])) if len(i) else np.zeros((0, 0))
        W = Ainv @ np.abs(A[np.ix_(i, k)])
        bnd = Hm[np.ix_(k, k)] + Hm[np.ix_(k, i)] @ W + W.T @ Hm[np.ix_(i, k)] + W.T @ Hm[np.ix_(i, i)] @ W
        dS = np.abs(S - S_ref)
        wS = (dS[dS > 0] / (C_H * EPS * bnd[dS > 0])).max() if (dS > 0).any() else 0.0      # (bnd = 0 and dS > 0: inf, fails)
        u = Ainv @ np.abs(R.b[i])
        bnd_g = R.bm[k] + Hm[np.ix_(k, i)] @ u + np.abs(A[np.ix_(k, i)]) @ (Ainv @ R.bm[i]) + W.T @ Hm[np.ix_(i, i)] @ u
        dg = np.abs(red["b"][live].reshape(-1) - g_ref)
        wg = (dg[dg > 0] / (C_H * EPS * bnd_g[dg > 0])).max() if (dg > 0).any() else 0.0
        _note("%s reduced matrix / bound" % key, wS)
        _note("%s reduced rhs / bound" % key, wg)
        assert wS <= 1.0, "reduced matrix differs by %.3g x its bound" % wS
        assert wg <= 1.0, "reduced right-hand side differs by %.3g x its bound" % wg
        # the PCG's SpMV on the reduced system (empty rows: x = 0 there)
        x = np.zeros((nr, 6)); x[live] = np.random.default_rng(nr).normal(size=(int(live.sum()), 6))
        y = p.apply(0, x, lam)
        dy = np.abs(y[live].reshape(-1) - S @ x[live].reshape(-1))
        by = C_H * EPS * (np.abs(S) @ np.abs(x[live].reshape(-1)))
        w = (dy[dy > 0] / by[dy > 0]).max() if (dy > 0).any() else 0.0
        _note("%s reduced SpMV / bound" % key, w)
        assert w <= 1.0, w
        assert np.all(y[~live] == 0)
        out.append(red)
    return out


@pytest.mark.parametrize("numbering", [1, 2])
def test_schur_reduced_system_chain_with_closures(capi, oracle, numbering):
    p, lin, R = _system(capi, oracle, chain_with_closures(), dict(reduced_numbering=numbering))
    try:
        reds = check_reduced(p, lin, R, "Schur 600/630 numbering=%d" % numbering)
        if numbering == 2:
            assert (reds[0]["sep_rows"] < 0).any(), "the strong numbering has no empty rows here"
        check_solve(p, oracle, chain_with_closures(), "Schur 600/630 numbering=%d" % numbering)
    finally:
        p.close()


def test_schur_everything_eliminated_system(capi, oracle):
    g = everything_eliminated()
    p, lin, R = _system(capi, oracle, g, {})
    try:
        red = p.reduced()
        assert red is not None and len(red["sep_rows"]) == 0
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------------------------ (d) preconditioner
def dense_operator(p, op, nrows, lam):
    """The operator as a dense matrix, one hook call per column."""
    M = np.zeros((6 * nrows, 6 * nrows))
    e = np.zeros((nrows, 6))
    for c in range(6 * nrows):
        e.flat[c] = 1.0
        M[:, c] = p.apply(op, e, lam).reshape(-1)
        e.flat[c] = 0.0
    return M


def test_block_jacobi_inverse(capi, oracle):
    """M^-1 x = blockdiag(A)^-1 x: per entry within C_H eps kappa(A_aa) (|A_aa^-1| |x|) (a backward-stable 6 x 6 inverse)."""
    p, lin, R = _system(capi, oracle, synth.make_pose_graph(300, 1200, seed=13), dict(preconditioner=0, schur_reduce=-1))
    try:
        lam = 1e-5 * lin["diagmax"]
        x = np.random.default_rng(1).normal(size=(R.nb, 6))
        y = p.apply(1, x, lam)
        A = (R.H + lam * sp.identity(6 * R.nb, format="csr")).tocsr()
        w = 0.0
        for a in range(R.nb):
            Aa = A[6 * a:6 * a + 6, 6 * a:6 * a + 6].toarray()
            inv = np.linalg.inv(Aa)
            tol = C_H * EPS * np.linalg.cond(Aa) * (np.abs(inv) @ np.abs(x[a]))
            w = max(w, (np.abs(y[a] - inv @ x[a]) / tol).max())
        _note("block-Jacobi M^-1 / bound", w)
        assert w <= 1.0, w
    finally:
        p.close()


# kappa(M^-1 A) measured on an MI355X (lambda_init); the assertions sit at twice these values
# additive: 60 / 180 graph (59 free vertices, one coarse level), eigenvalues 0.183 .. 2.91; multiplicative: C1 (100 / 300), 0.151 .. 2.91
KAPPA = {"additive": 15.94, "multiplicative": 19.25}


def _spectrum_case(capi, oracle, g, want_op, name):
    p, lin, R = _system(capi, oracle, g, dict(schur_reduce=-1))
    try:
        info = p.apply_info()
        assert info["op"] == want_op, info
        lam = 1e-5 * lin["diagmax"]
        M = dense_operator(p, 1, R.nb, lam)
        A = (R.H + lam * sp.identity(6 * R.nb, format="csr")).toarray()
        ev = np.linalg.eigvals(M @ A)
        scale = np.abs(ev).max()
        if want_op == 1:                                  # M and A SPD: a real spectrum, up to the round-off of eig
            assert np.abs(ev.imag).max() <= 1e-6 * scale, "M^-1 A has complex eigenvalues"
        assert ev.real.min() > 0, "M^-1 A has an eigenvalue with a real part <= 0"
        kappa = np.abs(ev).max() / np.abs(ev).min()
        _note("kappa(M^-1 A) %s" % name, kappa)
        print("\nkappa(M^-1 A) %s: %.4g (eigenvalues %.4g .. %.4g)" % (name, kappa, ev.real.min(), ev.real.max()))
        assert kappa <= 2 * KAPPA[name], kappa
        return M, A
    finally:
        p.close()


def test_additive_multilevel_is_spd_and_bounded(capi, oracle):
    """Additive multilevel operator (nb <= 64: one coarse level, no dense operator): symmetric to round-off - |M - M^T| <= C_H eps
    kappa(M) max|M|, a sum of inverses each taken backward-stably - positive definite, and kappa(M^-1 A) bounded."""
    M, A = _spectrum_case(capi, oracle, synth.make_pose_graph(60, 180, seed=60), 1, "additive")
    asym = np.abs(M - M.T).max() / (C_H * EPS * np.linalg.cond(M) * np.abs(M).max())
    _note("additive M symmetry / bound", asym)
    assert asym <= 1.0, asym
    assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0
    rng = np.random.default_rng(3)
    for _ in range(3):
        v = rng.normal(size=M.shape[0])
        assert v @ M @ v > 0


def test_multiplicative_operator_spectrum_bounded(capi, oracle):
    """The multiplicative cycle + Newton-Schulz operator of small graphs (not SPD by construction): real positive spectrum of M^-1 A and
    kappa bounded."""
    _spectrum_case(capi, oracle, synth.make_pose_graph(100, 300), 2, "multiplicative")


@pytest.mark.parametrize("name", ["additive", "multiplicative"])
def test_spectrum_extremes_are_the_reference_operators(capi, oracle, name):
    """The two graphs above once more, tied to the mathematics instead of a past run: kappa(M_ref^-1 A) of the float64 reference
    application (hierarchy_checks.apply_reference on the arrays the set-up kernels left, each of which test_pgo_hierarchy_gpu.py holds
    against its own float64 stage), computed on the CPU, and the device operator's extreme eigenvalues within | |dM| |A| |_2 of the
    reference's.  |dM| = the entrywise application bound, C_H eps x the absolute-value application of the unit vectors.  Derivation
    (Bauer-Fike for the symmetrised pencil): M A is similar to A^1/2 M A^1/2; for a symmetric perturbation E of M that matrix moves
    by A^1/2 E A^1/2, whose norm is the spectral radius of E A <= |E A|_2 <= | |E| |A| |_2, and the extreme eigenvalues of a symmetric
    matrix move by at most that (Weyl).  Both operators enter by their symmetric parts (the multiplicative one is symmetric to ~1e-9
    only, which moves an eigenvalue in second order), |sym(dM)| <= sym(|dM|)."""
    import hierarchy_checks as HC
    g = synth.make_pose_graph(60, 180, seed=60) if name == "additive" else synth.make_pose_graph(100, 300)
    p, lin, R = _system(capi, oracle, g, dict(schur_reduce=-1))
    try:
        assert p.apply_info()["op"] == (1 if name == "additive" else 2)
        h = p.hierarchy()
        lam = h["lam"]
        M = dense_operator(p, 1, R.nb, lam)
        n = 6 * R.nb
        lv0 = h["lv"][0]
        A = NP.bcsr_to_sparse(lv0["row_ptr"], lv0["col"], lv0["blk"], diag=lv0["G"] + lam * np.eye(6), nrows=R.nb).toarray()
        Mref = np.zeros((n, n)); B = np.zeros((n, n))
        e = np.zeros((R.nb, 6))
        for c in range(n):
            e.flat[c] = 1.0
            Mref[:, c] = HC.apply_reference(h, e).reshape(-1)
            B[:, c] = C_H * EPS * HC.apply_reference(h, e, absolute=True).reshape(-1)
            e.flat[c] = 0.0
        assert (np.abs(M - Mref) <= B).all(), "the device operator is not within the application bound of the reference's"
        Lc = np.linalg.cholesky(0.5 * (A + A.T))
        ev = np.linalg.eigvalsh(Lc.T @ (0.5 * (M + M.T)) @ Lc)
        ev_ref = np.linalg.eigvalsh(Lc.T @ (0.5 * (Mref + Mref.T)) @ Lc)
        margin = np.linalg.norm(0.5 * (B + B.T) @ np.abs(A), 2)
        kappa_ref = ev_ref[-1] / ev_ref[0]
        print("\nkappa(M_ref^-1 A) %s: %.6g (eigenvalues %.6g .. %.6g); device %.6g .. %.6g; margin %.3g" % (
            name, kappa_ref, ev_ref[0], ev_ref[-1], ev[0], ev[-1], margin))
        _note("kappa(M_ref^-1 A) %s" % name, kappa_ref)
        _note("extreme eigenvalues, device - reference / margin (%s)" % name, max(abs(ev[0] - ev_ref[0]), abs(ev[-1] - ev_ref[-1])) / margin)
        assert ev_ref[0] > 0
        assert abs(ev[0] - ev_ref[0]) <= margin and abs(ev[-1] - ev_ref[-1]) <= margin, (ev[0] - ev_ref[0], ev[-1] - ev_ref[-1], margin)
        assert kappa_ref <= 2 * KAPPA[name]
    finally:
        p.close()
