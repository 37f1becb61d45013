"""The reference helpers test_pgo_system_gpu.py leans on (np_reference: block-CSR assembly, dense Schur complement, step-error metric),
against plain numpy.linalg on small random SPD systems."""
import numpy as np
import pytest

import np_reference as NP


def _random_bcsr(rng, nb=7, extra=12):
    """A random symmetric block-CSR with one slot per 'edge' (pairs repeated: multi-edges), some neighbours fixed (col = -1), and the
    dense matrix it stands for."""
    pairs = [(a, a + 1) for a in range(nb - 1)] + [tuple(rng.choice(nb, 2, replace=False)) for _ in range(extra)]
    pairs += pairs[:3]                                                    # repeated pairs: several slots for one block
    rows = {a: [] for a in range(nb)}
    dense = np.zeros((6 * nb, 6 * nb))
    for a, c in pairs:
        B = rng.normal(size=(6, 6))
        rows[a].append((c, B)); rows[c].append((a, B.T))
        dense[6 * a:6 * a + 6, 6 * c:6 * c + 6] += B
        dense[6 * c:6 * c + 6, 6 * a:6 * a + 6] += B.T
    for a in range(0, nb, 3):
        rows[a].append((-1, rng.normal(size=(6, 6))))                    # a fixed neighbour: the slot's block is not part of H
    diag = np.zeros((nb, 6, 6))
    for a in range(nb):
        G = rng.normal(size=(6, 6))
        diag[a] = G @ G.T + 60 * np.eye(6)
        dense[6 * a:6 * a + 6, 6 * a:6 * a + 6] += diag[a]
    row_ptr = [0]; col = []; blk = []
    for a in range(nb):
        for c, B in sorted(rows[a], key=lambda t: t[0]):
            col.append(c); blk.append(B)
        row_ptr.append(len(col))
    return np.array(row_ptr), np.array(col), np.array(blk), diag, dense


def test_bcsr_assembly_sums_slots_and_skips_fixed():
    rng = np.random.default_rng(1)
    row_ptr, col, blk, diag, dense = _random_bcsr(rng)
    H = NP.bcsr_to_sparse(row_ptr, col, blk, diag=diag).toarray()
    assert np.allclose(H, dense, rtol=0, atol=1e-12)
    assert np.allclose(H, H.T, rtol=0, atol=1e-12)


@pytest.mark.parametrize("fault", ["drop", "duplicate"])
def test_bcsr_assembly_sees_a_dropped_or_duplicated_slot(fault):
    rng = np.random.default_rng(2)
    row_ptr, col, blk, diag, dense = _random_bcsr(rng)
    s = int(np.nonzero(col >= 0)[0][5])
    blk = blk.copy()
    blk[s] *= 0.0 if fault == "drop" else 2.0
    H = NP.bcsr_to_sparse(row_ptr, col, blk, diag=diag).toarray()
    assert np.abs(H - dense).max() > 1e-3


def test_schur_complement_matches_numpy():
    rng = np.random.default_rng(3)
    _, _, _, _, A = _random_bcsr(rng, nb=9)
    b = rng.normal(size=A.shape[0])
    keep = np.array([6, 1, 4])
    S, g = NP.schur_dense(A, b, keep)
    # the Schur complement's solution is the full solution on the kept blocks
    x = np.linalg.solve(A, b)
    xs = np.linalg.solve(S, g)
    assert np.allclose(xs, x[NP.block_index(keep)], rtol=1e-10, atol=1e-12)
    # and S is the inverse of the kept blocks of A^-1
    Ainv = np.linalg.inv(A)
    k = NP.block_index(keep)
    assert np.allclose(np.linalg.inv(S), Ainv[np.ix_(k, k)], rtol=1e-9, atol=1e-12)
    # nothing eliminated: the kept blocks themselves
    S2, g2 = NP.schur_dense(A, b, np.arange(9))
    assert np.array_equal(S2, A) and np.array_equal(g2, b)


def test_step_error_per_component():
    ref = np.zeros((4, 6))
    dx = ref.copy(); dx[2, 1] = -3e-6; dx[3, 5] = 2e-7; dx[0, 3] = -1e-7
    assert NP.step_error(dx, ref) == (3e-6, 2e-7)
    assert NP.step_error(np.zeros((0, 6)), np.zeros((0, 6))) == (0.0, 0.0)


def test_system_magnitudes_bound_the_system(oracle):
    """|H| <= S_H and |b| <= S_b entry by entry, S_H is exactly |H| where every term is non-negative, and the structure matches."""
    from uzliti_slam_amd import synth
    g = synth.make_pose_graph(60, 150, seed=3)
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    fixed, _ = oracle.set_fixed_nodes(fl["fixed"], fl["ij"])
    X = fl["poses"].reshape(-1, 3, 4); Z = fl["meas"].reshape(-1, 3, 4)
    J = [oracle.edge_jacobians(X[i], X[j], Z[k]) for k, (i, j) in enumerate(fl["ij"])]
    jac = (np.array([a for a, _ in J]), np.array([b for _, b in J]))
    H, b, _ = NP.build_system(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], jac=jac)
    Hm, bm = NP.system_magnitudes(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], jac)
    Hd, Hmd = H.toarray(), Hm.toarray()
    assert (np.abs(Hd) <= Hmd * (1 + 1e-12) + 1e-300).all()
    assert (np.abs(b) <= bm).all()
    assert np.array_equal(Hmd != 0, (Hmd != 0) & ((np.abs(Hd) > 0) | (Hmd > 0)))
    # the dense oracle system is the same matrix
    Hdo, bdo = oracle.build_dense(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"])
    assert (np.abs(Hdo - Hd) <= 1e3 * np.finfo(float).eps * Hmd + 1e-300).all()
    assert (np.abs(bdo - b) <= 1e3 * np.finfo(float).eps * bm).all()


# ------------------------------------------------------------------------------------------------------------------ multilevel hierarchy
# The float64 restatement of the preconditioner's hierarchy (np_reference.ml_*) against plain scipy, and the stage checks of
# hierarchy_checks.py against planted faults: what test_pgo_hierarchy_gpu.py holds the kernels to.
import scipy.sparse as sp

import hierarchy_checks as HC


def _bcsr_from_sparse(H, nb):
    """Block-CSR (one slot per nonzero off-diagonal block, columns ascending) and the diagonal blocks of a scalar sparse matrix."""
    Hd = H.toarray().reshape(nb, 6, nb, 6).transpose(0, 2, 1, 3)
    nz = np.abs(Hd).reshape(nb, nb, -1).max(2) > 0
    np.fill_diagonal(nz, False)
    r, c = np.nonzero(nz)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=nb))])
    return row_ptr, c, Hd[r, c], Hd[np.arange(nb), np.arange(nb)].copy()


@pytest.fixture(scope="module")
def free_graph(oracle):
    """A 203-vertex pose graph with NO fixed vertex (H is singular: its null space is the six rigid-body modes) as a block system."""
    from uzliti_slam_amd import synth
    g = synth.make_pose_graph(203, 700, seed=17)
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    fixed = np.zeros(203, np.uint8)
    X = fl["poses"].reshape(-1, 3, 4); Z = fl["meas"].reshape(-1, 3, 4)
    J = [oracle.edge_jacobians(X[i], X[j], Z[k]) for k, (i, j) in enumerate(fl["ij"])]
    jac = (np.array([a for a, _ in J]).reshape(-1, 6, 6), np.array([b for _, b in J]).reshape(-1, 6, 6))
    H, _, _ = NP.build_system(fl["poses"], fixed, fl["ij"], fl["meas"], fl["info"], fl["robust"], jac=jac)
    row_ptr, col, blk, hdiag = _bcsr_from_sparse(H, 203)
    return dict(H=H, row_ptr=row_ptr, col=col, blk=blk, hdiag=hdiag, t=X[:, :, 3].copy(), R=X[:, :, :3].copy(),
                lam=1e-5 * np.abs(H.diagonal()).max())


def _sparse_P(Pblk, fan):
    n = len(Pblk); nc = -(-n // fan)
    rr = 6 * np.arange(n)[:, None, None] + np.arange(6)[None, :, None] + np.zeros((1, 1, 6), np.int64)
    cc = 6 * (np.arange(n) // fan)[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), np.int64)
    return sp.coo_matrix((Pblk.ravel(), (rr.ravel(), cc.ravel())), shape=(6 * n, 6 * nc)).tocsr()


def test_galerkin_blocks_equal_the_dense_triple_product(free_graph):
    s = free_graph
    h, _ = HC.reference_hierarchy(s["row_ptr"], s["col"], s["blk"], s["hdiag"], s["t"], s["R"], s["lam"])
    assert h["levels"] == 2 and [lv["n"] for lv in h["lv"]] == [203, 26, 4]
    HC.check_structure(h)
    A = s["H"]
    for l in range(2):
        F, C = h["lv"][l], h["lv"][l + 1]
        P = _sparse_P(NP.ml_prolong_blocks(l, F["geo"]), C["fan"])
        want = (P.T @ A @ P).toarray()
        got = NP.bcsr_to_sparse(C["row_ptr"], C["col"], C["blk"], diag=C["G"], nrows=C["n"]).toarray()
        mag = (abs(P).T @ abs(A) @ abs(P)).toarray()
        assert (np.abs(got - want) <= 1e3 * np.finfo(float).eps * mag).all()
        Mw = (P.T @ (sp.identity(A.shape[0]) if l == 0 else sp.block_diag(list(F["M"]))) @ P).toarray()
        Mg = sp.block_diag(list(C["M"])).toarray()
        Mblock = np.kron(np.eye(C["n"]), np.ones((6, 6)))            # (M_l keeps the diagonal blocks of P^T M P only)
        assert np.allclose(Mg, Mw * Mblock, rtol=0, atol=1e-9 * np.abs(Mw).max())
        A = sp.csr_matrix(got)                                       # (the next level is held against ITS inputs)


def test_rigid_body_modes_are_in_the_range_of_the_prolongation(free_graph):
    """No fixed vertex, lambda = 0: A_0 P_1 e = 0 to round-off for every coarse vector that moves all aggregates by ONE world twist."""
    s = free_graph
    cen, geo = NP.ml_geometry(s["t"], s["R"], [1, 8])
    P = _sparse_P(NP.ml_prolong_blocks(0, geo[0]), 8)
    for k in range(6):
        tw = np.zeros(6); tw[k] = 1.0
        # the same world twist about every aggregate's own centroid: v_A = v + w x c_A
        e = np.tile(tw, (26, 1))
        e[:, :3] += np.cross(tw[3:], cen[1][:, :3])
        y = s["H"] @ (P @ e.reshape(-1))
        mag = abs(s["H"]) @ (abs(P) @ np.abs(e.reshape(-1)))
        assert (np.abs(y) <= 1e3 * np.finfo(float).eps * mag).all(), (k, np.abs(y).max())


@pytest.mark.parametrize("cl", [0, 1])
def test_application_equals_the_explicit_sum_of_matrices(free_graph, cl):
    s = free_graph
    h, _ = HC.reference_hierarchy(s["row_ptr"], s["col"], s["blk"], s["hdiag"], s["t"], s["R"], s["lam"], cl=cl, mult=0, top_max=8 if cl == 0 else 16)
    fans = HC.fans_of(h)
    L = h["levels"]
    Ps = [_sparse_P(NP.ml_prolong_blocks(l, h["lv"][l]["geo"]), fans[l + 1]).toarray() for l in range(L)]
    Ss = [NP.ml_dense_S(h["lv"][l]["Winv"], h["lv"][l]["n"]) for l in range(L)]
    M = h["top_inv"]
    for l in range(L - 1, -1, -1):
        M = Ss[l] + Ps[l] @ M @ Ps[l].T
    if cl:       # the dense operator enters as f32 values: compare against the same sum with Y_cl rounded
        Y = h["Cmat32"][:, :6 * h["lv"][1]["n"]].astype(np.float64)
        M = Ss[0] + Ps[0] @ Y @ Ps[0].T
    rng = np.random.default_rng(5)
    for _ in range(3):
        x = rng.normal(size=(h["rows"], 6))
        z = HC.apply_reference(h, x)
        mag = HC.apply_reference(h, x, absolute=True)
        assert (np.abs(z.reshape(-1) - M @ x.reshape(-1)) <= 1e3 * np.finfo(float).eps * mag.reshape(-1)).all()
        assert (np.abs(z) <= mag * (1 + 1e-12)).all()


def test_multiplicative_cycle_contracts_and_newton_schulz_keeps_it(free_graph):
    """eig(X_0 A) in (0, 1] when Y_{l+1} is exact, and after every Newton-Schulz step: the iteration contracts errors."""
    s = free_graph
    h, h0 = HC.reference_hierarchy(s["row_ptr"], s["col"], s["blk"], s["hdiag"], s["t"], s["R"], s["lam"])
    assert h["lv"][2]["n"] == 4 and h["cl"] == 1                       # (Y_2 = top_inv: exact)
    F = h["lv"][1]
    A = NP.ml_level_matrix(F["row_ptr"], F["col"], F["blk"], F["G"], F["M"], s["lam"])
    X = h0["lv"][1]["Y"]
    for k in range(3):
        ev = np.linalg.eigvals(X @ A)
        assert np.abs(ev.imag).max() <= 1e-8 and ev.real.min() > 0 and ev.real.max() <= 1 + 1e-9, (k, ev.real.min(), ev.real.max())
        X, _ = NP.ml_newton_schulz(X, A, 1)
    assert np.abs(X - h["lv"][1]["Y"]).max() > 0                       # (h holds two steps, X three)


def _worst(findings, stage):
    f = [x for x in findings if x.stage.startswith(stage)]
    assert f, stage
    return max(x.ratio for x in f)


def test_stage_checks_pass_on_the_reference_and_see_planted_faults(free_graph):
    """Every stage check of hierarchy_checks.py: below its bound on the reference's own hierarchy, and pushed over it by a factor >= 1e6
    (printed) by each fault planted on the reference side - a dropped Galerkin contribution, the last short aggregate's centroid taken
    over fan, a sibling coupling left out of W, a transposed sibling tile, a skipped Newton-Schulz step, a 16 x 16 tile of Q Y Q^T left out."""
    s = free_graph
    h, h0 = HC.reference_hierarchy(s["row_ptr"], s["col"], s["blk"], s["hdiag"], s["t"], s["R"], s["lam"])
    assert h["lv"][0]["n"] % 8 == 3                                       # the last aggregate of level 1 is short
    clean = HC.check_geometry(h, s["t"], s["R"]) + HC.check_galerkin(h) + HC.check_inverses(h) + HC.check_dense(h, h0)
    HC.check_cmat32(h)
    for f in clean:
        assert f.ratio <= 1.0, f
    assert {f.stage for f in clean} >= {"geometry cen", "galerkin blk", "sibling inverses", "top inverse", "multiplicative cycle X0", "Newton-Schulz"}
    assert not [f for f in clean if "symmetry" in f.stage]
    ha, _ = HC.reference_hierarchy(s["row_ptr"], s["col"], s["blk"], s["hdiag"], s["t"], s["R"], s["lam"], mult=0)
    for f in HC.check_dense(ha):
        assert f.stage == "additive dense" and f.ratio <= 1.0, f
    nslots1 = int((h["lv"][1]["col"] >= 0).sum())
    factors = {
        "galerkin level 1: last contribution dropped": _worst(HC.check_galerkin(h, fault=(0, ("drop", int((h["lv"][0]["col"] >= 0).sum()) - 1))), "galerkin"),
        "galerkin level 2: contribution %d dropped" % (nslots1 // 2): _worst(HC.check_galerkin(h, fault=(1, ("drop", nslots1 // 2))), "galerkin"),
        "sibling inverses level 0: one coupling slot of W left out": _worst(HC.check_inverses(h, fault=(0, ("drop", 40))), "sibling inverses"),
        "sibling inverses level 1: one coupling slot of W left out": _worst(HC.check_inverses(h, fault=(1, ("drop", 7))), "sibling inverses"),
        "geometry: short aggregate's centroid over fan": _worst(HC.check_geometry(h, s["t"], s["R"], fault=("fan", 1)), "geometry"),
        "multiplicative cycle: sibling tile (1, 0) of aggregate 2 transposed": _worst(HC.check_dense(h, h0, fault=("transpose", 2, 1, 0)), "multiplicative cycle X0"),
        "additive dense: sibling tile (1, 0) of aggregate 2 transposed": _worst(HC.check_dense(ha, fault=("transpose", 2, 1, 0)), "additive dense"),
        "Newton-Schulz: last step skipped": _worst(HC.check_dense(h, h0, fault=("skip", 1)), "Newton-Schulz"),
        "multiplicative cycle: edge tile (3, 9) of Q Y Q^T left out": _worst(HC.check_dense(h, h0, fault=("tile", 3, 9)), "multiplicative cycle X0"),
    }
    print()
    for k, v in factors.items():
        print("  planted fault / bound  %-70s %.3e" % (k, v))
    for k, v in factors.items():
        assert v >= 1e6, (k, v)
    # the f32 copy is exact: one flipped bit fails
    hb = dict(h, Cmat32=h["Cmat32"].copy())
    hb["Cmat32"].view(np.uint32)[5, 7] ^= 1
    with pytest.raises(AssertionError):
        HC.check_cmat32(hb)
    # an application with one sibling tile transposed
    x = np.random.default_rng(9).normal(size=(h["rows"], 6))
    z = HC.apply_reference(h, x)
    assert HC.check_apply(h, x, z).ratio <= 1.0
    hw = dict(h, lv=[dict(v) for v in h["lv"]])
    W = hw["lv"][0]["Winv"].copy(); W[3, 6:12, 0:6] = W[3, 6:12, 0:6].T.copy(); hw["lv"][0]["Winv"] = W
    fa = HC.check_apply(hw, x, z).ratio
    print("  planted fault / bound  %-70s %.3e" % ("application: level-0 sibling tile transposed", fa))
    assert fa >= 1e6
