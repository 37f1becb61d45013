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
